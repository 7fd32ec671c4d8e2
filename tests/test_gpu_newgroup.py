"""k_newgroup / epx_predict_new_group / Master.predict_new_group on the device: the posterior predictive of groups that
were not in the data, against newgroup.predict_new_group_host (NumPy) on the same draws.  Need a real MI355X.

Tolerances (derived, not tuned): those of tests/test_gpu_predict.py with S read as N (N 2^-53 stays below 1e-11 up to
N = 10^5) and A_i, the reach of |alpha| + sum_j |x_ij beta_j| over the pool, enlarged by the latents' reach:
A_i = max_t (|mu_a| + sum_j |x_ij mu_bj| + 8.7 (sigma_a + sum_j |x_ij| sigma_bj)); 8.7 bounds |z| for both families at
u >= 2^-54 (sqrt(-2 log 2^-54) = 8.66, -log 2^-53 = 36.7 for the Laplace case is reached with probability 2^-52 only: its
8.7 is exceeded with probability e^-8.7, and then by little against three orders of margin).  MEAN and F_MEAN at
rtol 1e-9 + atol 1e-12 A_i, F_M2 at rtol 1e-9, LPD at rtol 1e-9 + atol 1e-10 A_i, GLPD at rtol 1e-9 + atol 1e-10 sum_{i in g}
A_i.  Latents: the angle 2 pi u2 carries about 7e-16 absolute error and the radius is at most 8.7; with <= 2 ulp each for
log, sqrt, sincos and log1p the worst case is about 6e-15: atol = rtol = 1e-13, one order above."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from epstan_amd import _lib, fit, newgroup, site_params    # noqa: E402
from epstan_amd.engine import HipEngine, MODEL_IDS, is_gauss  # noqa: E402
from test_gpu_parity import _site_problem, _engine_with_cavity, _group_problem   # noqa: E402

RTOL = 1e-9
MEAN, F_MEAN, F_M2, LPD = site_params.PR_MEAN, site_params.PR_F_MEAN, site_params.PR_F_M2, site_params.PR_LPD
LABELS = np.array([7, 0, 3, 100000, 12])                 # not contiguous, not sorted
PER_GROUP = [3, 0, 16, 17, 65]                           # an empty group, a full tile, one past a tile, one past a 64-row block


def _spec(model):
    return MODEL_IDS[model] % 5, is_gauss(model)


def _scale(model, D, phi, Xn):
    """A_i of every new row over the pool phi (T, d), the latents' reach included."""
    mid, gauss = _spec(model)
    b = phi[:, (1 if gauss else 0):]
    zero = np.zeros((phi.shape[0], D))
    if mid == 0:
        a0, sa, b0, sb = 0.0, np.exp(b[:, 0]), np.abs(b[:, 1:1 + D]), zero
    elif mid == 1:
        a0, sa, b0, sb = 0.0, np.exp(b[:, 0]), zero, np.exp(b[:, 1])[:, None] + zero
    elif mid == 2:
        a0, sa, b0, sb = 0.0, np.exp(b[:, 0]), zero, np.exp(b[:, 1:1 + D])
    else:
        a0, sa, b0, sb = np.abs(b[:, 0]), np.exp(b[:, 1]), np.abs(b[:, 2:2 + D]), np.exp(b[:, 2 + D:2 + 2 * D])
    A = (a0 + 8.7 * sa)[:, None] + (b0 + 8.7 * sb).dot(np.abs(Xn).T)
    return np.maximum(1.0, A.max(axis=0))


def _close(got, exp, rtol, atol, what):
    err = np.abs(got - exp)
    bound = atol + rtol * np.abs(exp)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / bound)             # (a group without rows: 0 against a bound of 0)
    print('%s: largest error %.3e, largest error / bound %.3e' % (what, err.max(), ratio.max()))
    assert np.all(err <= bound), what


def _assert_close(model, D, phi, Xn, gidx, y, got, exp, what=''):
    """(rows, glpd, N) of the device against the same of the host (or of a merge) on the pool phi (count, S, d)."""
    A = _scale(model, D, phi.reshape(-1, phi.shape[-1]), Xn)
    assert got[2] == exp[2] and got[0].shape == exp[0].shape and got[1].shape == exp[1].shape
    if Xn.shape[0]:
        assert np.all(np.isfinite(got[0][:, :3])), what
        _close(got[0][:, MEAN], exp[0][:, MEAN], RTOL, 1e-12 * A, what + ' MEAN')
        _close(got[0][:, F_MEAN], exp[0][:, F_MEAN], RTOL, 1e-12 * A, what + ' F_MEAN')
        _close(got[0][:, F_M2], exp[0][:, F_M2], RTOL, 0.0, what + ' F_M2')
    if y is None:
        assert np.all(np.isnan(got[0][:, LPD])) and np.all(np.isnan(got[1])), what
    else:
        assert np.all(np.isfinite(got[0][:, LPD])) and np.all(np.isfinite(got[1])), what
        if Xn.shape[0]:
            _close(got[0][:, LPD], exp[0][:, LPD], RTOL, 1e-10 * A, what + ' LPD')
        Ag = np.bincount(gidx, weights=A, minlength=got[1].shape[0])
        _close(got[1], exp[1], RTOL, 1e-10 * Ag, what + ' GLPD')


def _responses(model, rng, n):
    return 0.4 + rng.randn(n) if is_gauss(model) else (rng.rand(n) < 0.5).astype(np.float64)


def _rows(model, D, rng, per_group=PER_GROUP):
    """New rows with their groups mixed through each other."""
    gidx = rng.permutation(np.repeat(np.arange(len(per_group)), per_group)).astype(np.int32)
    n = gidx.shape[0]
    return 1.5 * rng.randn(n, D) / np.sqrt(D), gidx, _responses(model, rng, n)


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


# ------------------------------------------------------------------ (a) the latents
@pytest.mark.parametrize('model,D', [('m1b_sg', 3), ('m4b_sg', 1), ('m4b_sg', 4), ('m4b_sg', 128), ('m5b_sg', 4),
                                     ('m5a_sg', 3)])
def test_latents_match_the_host_stream(model, D):
    mid, _ = _spec(model)
    seed, label, t0, nt, R = 2 ** 45 + 17, 100000, 2 ** 31 - 3, 7, 3             # the pooled draws straddle 2^31
    E = newgroup.n_latents(mid, D)
    out = np.full((nt, R, E), np.nan)
    _lib.check(_lib.load().epx_newgroup_latents(0, MODEL_IDS[model], D, ctypes.c_uint64(seed), label, t0, nt, R,
                                                _lib.dptr(out)))
    exp = newgroup.latents_host(mid, D, seed, label, t0 + np.arange(nt), R)
    assert out.shape == exp.shape and np.all(np.isfinite(out))
    err = np.abs(out - exp)
    print('%s D=%d: largest latent error %.3e (bound 1e-13 (1 + |z|)), largest |z| %.3f' % (model, D, err.max(), np.abs(exp).max()))
    np.testing.assert_allclose(out, exp, rtol=1e-13, atol=1e-13)
    again = np.zeros_like(out)
    _lib.check(_lib.load().epx_newgroup_latents(0, MODEL_IDS[model], D, ctypes.c_uint64(seed), label, t0, nt, R,
                                                _lib.dptr(again)))
    assert again.tobytes() == out.tobytes()
    other = np.zeros_like(out)                           # another label: another stream
    _lib.check(_lib.load().epx_newgroup_latents(0, MODEL_IDS[model], D, ctypes.c_uint64(seed), label + 1, t0, nt, R,
                                                _lib.dptr(other)))
    assert np.all(other != out)
    # the far end of the range, and a range that leaves it
    last = np.zeros((1, R, E))
    _lib.check(_lib.load().epx_newgroup_latents(0, MODEL_IDS[model], D, ctypes.c_uint64(seed), label, 2 ** 32 - 1, 1, R,
                                                _lib.dptr(last)))
    np.testing.assert_allclose(last, newgroup.latents_host(mid, D, seed, label, [2 ** 32 - 1], R), rtol=1e-13, atol=1e-13)
    lib = _lib.load()
    for args, msg in (((0, MODEL_IDS[model], D, ctypes.c_uint64(seed), label, 2 ** 32 - 1, 2, R), b'outside [0,2^32)'),
                      ((0, MODEL_IDS[model], D, ctypes.c_uint64(seed), -1, 0, 2, R), b'negative'),
                      ((0, MODEL_IDS[model], 129, ctypes.c_uint64(seed), label, 0, 2, R), b'D = 129 columns'),
                      ((0, 10, D, ctypes.c_uint64(seed), label, 0, 2, R), b'unknown model'),
                      ((0, MODEL_IDS[model], D, ctypes.c_uint64(seed), label, 0, 2, 1025), b'R must be in 1..1024')):
        assert lib.epx_newgroup_latents(*(args + (_lib.dptr(last),))) != 0
        assert msg in lib.epx_last_error(), lib.epx_last_error()


# ------------------------------------------------------------------ (b) injected draws, every model family
@pytest.mark.parametrize('model', ['m1b_sg', 'm2b_sg', 'm3b_sg', 'm4b_sg', 'm5b_sg', 'm1a_sg', 'm4a_sg'])
@pytest.mark.parametrize('D,S,R', [(1, 21, 1), (3, 16, 2), (4, 33, 3), (32, 100, 1), (128, 17, 2)])
def test_injected_draws_match_the_host_statement(model, D, S, R):
    K = 5
    mid, gauss = _spec(model)
    X, y, k_lim, _, _, d, P = _site_problem(model, D, 7, 300 + D, K=K)
    eng = HipEngine(model, X, y, k_lim)
    assert eng.P == P and eng.d == d
    rng = np.random.RandomState(7 + D)
    theta = 0.5 * rng.randn(K, S, P) + 0.3
    theta[:, :, d:] = np.nan                              # only phi of a record may be read
    Xn, gidx, yn = _rows(model, D, rng)
    seed, t0 = 2 ** 40 + D, 1000
    got = eng.predict_new_group(Xn, gidx, LABELS, yn, seed=seed, t0=t0, R=R, theta=theta)
    assert got[0].shape == (101, 4) and got[1].shape == (5,) and got[2] == K * S * R
    exp = newgroup.predict_new_group_host(mid, D, gauss, theta[:, :, :d], Xn, gidx, LABELS, yn, seed, t0, R)
    _assert_close(model, D, theta[:, :, :d], Xn, gidx, yn, got, exp, '%s D=%d S=%d R=%d' % (model, D, S, R))
    assert got[1][1] == 0.0                               # the group without rows
    if gauss:
        assert got[0][:, MEAN].tobytes() == got[0][:, F_MEAN].tobytes()
    else:
        assert np.all((got[0][:, MEAN] > 0) & (got[0][:, MEAN] < 1))
    bare = eng.predict_new_group(Xn, gidx, LABELS, None, seed=seed, t0=t0, R=R, theta=theta)
    assert np.all(np.isnan(bare[0][:, LPD])) and np.all(np.isnan(bare[1]))
    assert bare[0][:, :3].tobytes() == got[0][:, :3].tobytes()
    eng.close()


def test_a_multi_group_context_reads_phi_alone():
    """A context of sites with several groups (record stride P of the widest site) against the `_sg` context on the same
    phi: the same bytes."""
    D, S, R = 3, 33, 2
    groups = [[9], [8, 7, 9], [10, 6]]
    X, y, k_lim, g_cnt, g_lim, _, _, d = _group_problem('m4b', D, groups, 23)
    multi = HipEngine('m4b', X, y, k_lim, g_cnt=g_cnt, g_lim=g_lim)
    Xs, ys, ks, _, _, ds, Ps = _site_problem('m4b_sg', D, 7, 3, K=3)
    single = HipEngine('m4b_sg', Xs, ys, ks)
    assert d == ds == multi.d and multi.P > Ps
    rng = np.random.RandomState(3)
    phi = 0.5 * rng.randn(3, S, d) + 0.3
    th_m, th_s = np.full((3, S, multi.P), np.nan), np.full((3, S, Ps), np.nan)
    th_m[:, :, :d], th_s[:, :, :d] = phi, phi
    Xn, gidx, yn = _rows('m4b', D, rng)
    a = multi.predict_new_group(Xn, gidx, LABELS, yn, seed=5, t0=17, R=R, theta=th_m)
    b = single.predict_new_group(Xn, gidx, LABELS, yn, seed=5, t0=17, R=R, theta=th_s)
    assert _same(a, b)
    exp = newgroup.predict_new_group_host(3, D, False, phi, Xn, gidx, LABELS, yn, 5, 17, R)
    _assert_close('m4b', D, phi, Xn, gidx, yn, a, exp, 'multi-group context')
    multi.close()
    single.close()


# ------------------------------------------------------------------ (c) invariances
def test_invariances_device_draws_sub_ranges_and_merged_halves():
    D, K = 4, 6
    X, y, k_lim, Oms, mus, d, P = _site_problem('m4b_sg', D, 40, 41, K=K, tight=4.0)
    eng, _, _ = _engine_with_cavity('m4b_sg', X, y, k_lim, Oms, mus)
    rng = np.random.RandomState(2)
    Xn, gidx, yn = _rows('m4b_sg', D, rng)
    kw = dict(seed=99, R=2)
    with pytest.raises(_lib.EpxError, match='no draws yet'):            # nothing sampled yet
        eng.predict_new_group(Xn, gidx, LABELS, yn, **kw)
    assert b'no draws yet' in eng.lib.epx_last_error()
    opts = HipEngine.sampler_opts(chains=4, iter=24, warmup=None, init='random')
    eng.sample_batch(np.arange(11, 11 + K, dtype=np.int64), opts)
    S = eng.num_draws()
    got = eng.predict_new_group(Xn, gidx, LABELS, yn, **kw)
    assert got[2] == K * S * 2
    assert _same(got, eng.predict_new_group(Xn, gidx, LABELS, yn, **kw))              # twice: the same bits
    draws = np.stack([np.ascontiguousarray(eng.get_draws(k, all_params=True)) for k in range(K)])
    assert _same(got, eng.predict_new_group(Xn, gidx, LABELS, yn, theta=draws, **kw))  # device draws against injected
    exp = newgroup.predict_new_group_host(3, D, False, draws[:, :, :d], Xn, gidx, LABELS, yn, 99, 0, 2)
    _assert_close('m4b_sg', D, draws[:, :, :d], Xn, gidx, yn, got, exp, 'device draws')
    # a subset of the rows of one group (the others whole): the per-row columns keep their bits
    keep = np.ones(len(gidx), dtype=bool)
    keep[np.nonzero(gidx == 4)[0][::3]] = False
    sub = eng.predict_new_group(Xn[keep], gidx[keep], LABELS, yn[keep], **kw)
    assert sub[0].tobytes() == got[0][keep].tobytes()
    assert sub[1][[0, 1, 2, 3]].tobytes() == got[1][[0, 1, 2, 3]].tobytes() and sub[1][4] != got[1][4]
    # a subset of the groups: their rows and their joint terms keep their bits
    keep = np.isin(gidx, [0, 3])
    dense = np.where(gidx[keep] == 3, 1, 0).astype(np.int32)
    sub = eng.predict_new_group(Xn[keep], dense, LABELS[[0, 3]], yn[keep], **kw)
    assert sub[0].tobytes() == got[0][keep].tobytes() and sub[1].tobytes() == got[1][[0, 3]].tobytes()
    # a sub-range of the sites against the same draws injected, at the matching t0
    part = eng.predict_new_group(Xn, gidx, LABELS, yn, k0=2, count=3, t0=2 * S, **kw)
    assert _same(part, eng.predict_new_group(Xn, gidx, LABELS, yn, k0=0, count=3, t0=2 * S, theta=draws[2:5], **kw))
    assert part[2] == 3 * S * 2 and not _same(part, eng.predict_new_group(Xn, gidx, LABELS, yn, k0=2, count=3, t0=0, **kw))
    # two halves of the sites merged against the whole
    halves = [eng.predict_new_group(Xn, gidx, LABELS, yn, k0=k0, count=3, t0=k0 * S, **kw) for k0 in (0, 3)]
    _assert_close('m4b_sg', D, draws[:, :, :d], Xn, gidx, yn, newgroup.merge(halves), got, 'merged halves')
    # stale sites
    eng.sample_batch(np.array([5, 6], dtype=np.int64), opts, k0=1, count=2)     # only sites 1, 2 are current now
    eng.predict_new_group(Xn, gidx, LABELS, yn, k0=1, count=2, t0=S, **kw)
    with pytest.raises(_lib.EpxError, match='left draws of sites'):
        eng.predict_new_group(Xn, gidx, LABELS, yn, **kw)
    eng.close()


def test_a_pool_of_many_chunks_of_more_than_the_smallest_size():
    """N = 72000 members: 4500 slabs in chunks of 18 (the chunk rule leaves its floor of 16), 250 chunks walked by a
    capped grid and merged in order; the last chunk is partial."""
    D, K, S, R = 2, 6, 1500, 8
    X, y, k_lim, _, _, d, P = _site_problem('m5b_sg', D, 7, 8, K=K)
    eng = HipEngine('m5b_sg', X, y, k_lim)
    rng = np.random.RandomState(12)
    theta = 0.4 * rng.randn(K, S, P) + 0.2
    Xn, gidx, yn = _rows('m5b_sg', D, rng, [9, 11])
    got = eng.predict_new_group(Xn, gidx, [4, 9], yn, seed=3, t0=2 ** 32 - K * S, R=R, theta=theta)
    assert got[2] == 72000
    assert _same(got, eng.predict_new_group(Xn, gidx, [4, 9], yn, seed=3, t0=2 ** 32 - K * S, R=R, theta=theta))
    exp = newgroup.predict_new_group_host(4, D, False, theta[:, :, :d], Xn, gidx, [4, 9], yn, 3, 2 ** 32 - K * S, R)
    _assert_close('m5b_sg', D, theta[:, :, :d], Xn, gidx, yn, got, exp, 'N = 72000')
    eng.close()


# ------------------------------------------------------------------ (d) saturation
def test_saturated_logits_and_vanishing_scales():
    D, S, R = 2, 21, 2
    X, y, k_lim, _, _, d, P = _site_problem('m4b_sg', D, 7, 5, K=2)
    eng = HipEngine('m4b_sg', X, y, k_lim)
    Xn = np.random.RandomState(1).randn(6, D)
    yn = np.array([1.0, 0.0, 1.0, 1.0, 0.0, 1.0])
    gidx = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    for mu_a in (750.0, -750.0):
        theta = np.zeros((2, S, P))                                     # [mu_a, log sigma_a, mu_b, log sigma_b | ...]
        theta[:, :, 0] = mu_a
        theta[:, :, 1], theta[:, :, 2 + D:2 + 2 * D] = -800.0, -800.0
        got = eng.predict_new_group(Xn, gidx, [1, 2], yn, seed=4, R=R, theta=theta)
        exp = newgroup.predict_new_group_host(3, D, False, theta[:, :, :d], Xn, gidx, [1, 2], yn, 4, 0, R)
        print(mu_a, got[0], got[1])
        assert np.all(got[0][:, MEAN] == (1.0 if mu_a > 0 else 0.0))
        assert np.all(got[0][:, F_MEAN] == mu_a) and np.all(got[0][:, F_M2] == 0.0)
        assert np.all(np.isfinite(got[0][:, LPD])) and np.all(np.isfinite(got[1]))
        np.testing.assert_allclose(got[0][:, LPD], exp[0][:, LPD], rtol=1e-12)
        np.testing.assert_allclose(got[1], exp[1], rtol=1e-12)
        wrong = yn != (1.0 if mu_a > 0 else 0.0)
        np.testing.assert_allclose(got[0][wrong, LPD], -750.0, rtol=1e-12)
        np.testing.assert_allclose(got[1], [-750.0 * wrong[:3].sum(), -750.0 * wrong[3:].sum()], rtol=1e-12)
    # wide latents: sigma_a = e^5; everything stays finite, and close to the host's
    rng = np.random.RandomState(5)
    theta = 0.3 * rng.randn(2, S, P)
    theta[:, :, 1] = 5.0
    theta[:, :, 2 + D:2 + 2 * D] = 2.0
    got = eng.predict_new_group(Xn, gidx, [1, 2], yn, seed=4, R=R, theta=theta)
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    exp = newgroup.predict_new_group_host(3, D, False, theta[:, :, :d], Xn, gidx, [1, 2], yn, 4, 0, R)
    _assert_close('m4b_sg', D, theta[:, :, :d], Xn, gidx, yn, got, exp, 'wide latents')
    eng.close()


# ------------------------------------------------------------------ (e) errors, not faults
def test_bad_arguments_are_errors():
    D, S = 3, 8
    X, y, k_lim, _, _, d, P = _site_problem('m4b_sg', D, 7, 23, K=3)
    eng = HipEngine('m4b_sg', X, y, k_lim)
    theta = np.zeros((3, S, P))
    Xn, yn = np.ones((6, D)), np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0])
    gidx = np.array([0, 2, 0, 1, 1, 0], dtype=np.int32)
    labels = [5, 6, 7]
    ok = eng.predict_new_group(Xn, gidx, labels, yn, theta=theta)
    assert ok[0].shape == (6, 4) and ok[1].shape == (3,) and ok[2] == 24

    def refused(match, **kw):
        args = dict(Xn=Xn, gidx=gidx, labels=labels, y=yn, theta=theta)
        args.update(kw)
        with pytest.raises(_lib.EpxError, match=match):
            eng.predict_new_group(**args)
        assert eng.lib.epx_last_error()

    for k0, count in ((-1, 2), (2, 2), (0, 0), (3, 1)):
        refused('site range', k0=k0, count=count, theta=theta[:max(count, 0)])
    refused(r'R must be in 1\.\.1024 \(got 0\)', R=0)
    refused(r'R must be in 1\.\.1024 \(got 1025\)', R=1025)
    refused(r'outside \[0,2\^32\)', t0=2 ** 32 - 3 * S + 1)
    refused('t0 = -1', t0=-1)
    assert eng.predict_new_group(Xn, gidx, labels, yn, theta=theta, t0=2 ** 32 - 3 * S)[2] == 24
    refused('row 1: group 3 outside', gidx=np.array([0, 3, 0, 1, 1, 0]))
    refused('row 0: group -1 outside', gidx=np.array([-1, 2, 0, 1, 1, 0]))
    refused('row 0: group 0 outside', gidx=None, labels=[])
    refused('group 1: label -4 is negative', labels=[5, -4, 7])
    refused('row 3: y = 0.5', y=np.where(np.arange(6) == 3, 0.5, yn))
    refused('row 2: y = nan', y=np.where(np.arange(6) == 2, np.nan, yn))
    refused('no draws yet', theta=None)
    out = np.full((1, 4), 7.0)                                          # n = 0: nothing launched, nothing written
    outg = np.full(3, 7.0)
    N = ctypes.c_longlong()
    lab = np.array(labels, dtype=np.int32)
    _lib.check(eng.lib.epx_predict_new_group(eng.ctx, 0, 3, ctypes.c_uint64(1), 0, 2, 0, None, None, None, 3,
                                             lab.ctypes.data_as(_lib.c_int32_p), _lib.dptr(theta), S, _lib.dptr(out),
                                             _lib.dptr(outg), ctypes.byref(N)))
    assert N.value == 3 * S * 2 and np.all(out == 7.0) and np.all(outg == 7.0)
    eng.close()

    Xg, yg, kg, _, _, _, Pg = _site_problem('m4a_sg', D, 7, 23, K=1)    # the Gaussian family: finite responses
    eng = HipEngine('m4a_sg', Xg, yg, kg)
    with pytest.raises(_lib.EpxError, match='row 4: y = inf'):
        eng.predict_new_group(Xn, gidx, labels, np.where(np.arange(6) == 4, np.inf, yn), theta=np.zeros((1, S, Pg)))
    eng.close()

    Xw, yw, kw, _, _, _, Pw = _site_problem('m1b_sg', 129, 4, 1, K=1)   # more columns than a row tile takes
    eng = HipEngine('m1b_sg', Xw, yw, kw)
    with pytest.raises(_lib.EpxError, match='D = 129 columns, at most 128'):
        eng.predict_new_group(np.ones((2, 129)), None, [0], None, theta=np.zeros((1, S, Pw)))
    eng.close()


# ------------------------------------------------------------------ (f) Master.predict_new_group on the device
@pytest.mark.parametrize('J,K', [(4, 4), (5, 3)])
def test_master_predict_new_group_on_the_device(J, K):
    D, R = 3, 2
    conf = fit.configurations(J=J, D=D, K=K, npg=30, siter=40, run_ep=True, damp=0.4)
    M = fit.main('m4b', conf, ret_master=True)
    assert isinstance(M.engine, HipEngine)
    assert M.run(2, verbose=False, calc_moments=False, seed=5) == 0
    rng = np.random.RandomState(J)
    n = 40
    Xn = rng.randn(n, D)
    group = rng.permutation(np.repeat([31, 2, 500000], [20, 3, 17]))
    yn = (rng.rand(n) < 0.5).astype(int)
    res = M.predict_new_group(Xn, group, y_new=yn, R=R, seed=77)
    S = M.engine.num_draws()
    N = K * S * R
    assert res['n'] == N and list(res['groups']) == [2, 31, 500000] and res['mean'].shape == (n,)
    assert np.all((res['mean'] > 0) & (res['mean'] < 1)) and np.all(res['f_var'] > 0)
    phi = np.stack([np.ascontiguousarray(M.engine.get_draws(k)) for k in range(K)])
    gidx = np.searchsorted(res['groups'], group)
    exp = newgroup.predict_new_group_host(3, D, False, phi, Xn, gidx, res['groups'], yn.astype(float), 77, 0, R)
    got = (np.stack([res['mean'], res['f_mean'], res['f_var'] * (N - 1), res['lpd']], axis=1), res['group_lpd'], N)
    _assert_close('m4b_sg', D, phi, Xn, gidx, yn, got, exp, 'J=%d K=%d' % (J, K))
    assert np.all(np.isfinite(res['group_lpd']))
    for i, g in enumerate(res['groups']):                               # the shared latents make them differ
        assert abs(res['lpd'][group == g].sum() - res['group_lpd'][i]) > 1e-6
    shuffle = rng.permutation(n)                                        # the caller's row order
    res2 = M.predict_new_group(Xn[shuffle], group[shuffle], y_new=yn[shuffle], R=R, seed=77)
    for key in ('mean', 'f_mean', 'f_var', 'lpd'):
        assert res2[key].tobytes() == res[key][shuffle].tobytes()
    bare = M.predict_new_group(Xn, group, R=R, seed=77)
    assert bare['lpd'] is None and bare['group_lpd'] is None and bare['f_mean'].tobytes() == res['f_mean'].tobytes()
