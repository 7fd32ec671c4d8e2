"""k_predict / epx_predict / Master.predict on the device: the posterior predictive of new rows from draws in device
memory, against site_params.predict_host (NumPy) on the same draws.  Need a real MI355X.

Tolerances (derived, not tuned): f is a dot product of at most 129 terms, |df| <= 129 2^-53 A_i with
A_i = max_s (|alpha| + sum_j |x_ij beta_j|); a mean over S <= 400 terms adds S 2^-53 relative; |d sigmoid / df| <= 1/4 and
|d ll / df| <= 1 for the Bernoulli-logit models.  Hence MEAN and F_MEAN at rtol 1e-9 + atol 1e-12 max(1, A_i), F_M2 at
rtol 1e-9, LPD at rtol 1e-9 + atol 1e-10 max(1, A_i) (the extra factor covers (y - f) / sigma^2 of the Gaussian models at
sigma >~ 0.3): three or more orders of margin over the bound."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from epstan_amd import _lib, fit, site_params               # noqa: E402
from epstan_amd.engine import HipEngine, MODEL_IDS, is_gauss  # noqa: E402
from test_gpu_parity import _site_problem, _engine_with_cavity, _group_problem   # noqa: E402

RTOL = 1e-9
MEAN, F_MEAN, F_M2, LPD = site_params.PR_MEAN, site_params.PR_F_MEAN, site_params.PR_F_M2, site_params.PR_LPD


def _spec(model):
    return MODEL_IDS[model] % 5, is_gauss(model)


def _scale(model, D, ng, theta_k, Xn, group):
    """A_i = max_s (|alpha_g(s)| + sum_j |x_ij beta_gj(s)|) of every new row."""
    mid, gauss = _spec(model)
    dr = site_params.named_draws(mid, D, ng, gauss, False, theta_k, ['alpha', 'beta'])
    a, b = np.abs(dr['alpha']), np.abs(dr['beta'])
    bg = b[:, None, :] if b.ndim == 2 else b[:, group, :]                # (S, 1 or n, D)
    return (a[:, group] + (bg * np.abs(Xn)[None, :, :]).sum(axis=2)).max(axis=0)


def _close(got, exp, rtol, atol, what):
    err = np.abs(got - exp)
    bound = atol + rtol * np.abs(exp)
    print('%s: largest error %.3e, largest error / bound %.3e' % (what, err.max(), (err / bound).max()))
    assert np.all(err <= bound), what


def _assert_site(model, D, ng, theta_k, Xn, group, y, got, what=''):
    """The rows of ONE site against predict_host on the same draws."""
    if Xn.shape[0] == 0:
        return
    mid, gauss = _spec(model)
    group = np.zeros(Xn.shape[0], dtype=np.int64) if group is None else np.asarray(group)
    exp = site_params.predict_host(mid, D, ng, gauss, theta_k, Xn, group, y)
    A = np.maximum(1.0, _scale(model, D, ng, theta_k, Xn, group))
    assert got.shape == exp.shape and np.all(np.isfinite(got[:, :3]))
    _close(got[:, MEAN], exp[:, MEAN], RTOL, 1e-12 * A, what + ' MEAN')
    _close(got[:, F_MEAN], exp[:, F_MEAN], RTOL, 1e-12 * A, what + ' F_MEAN')
    _close(got[:, F_M2], exp[:, F_M2], RTOL, 0.0, what + ' F_M2')
    if y is None:
        assert np.all(np.isnan(got[:, LPD])), what
    else:
        assert np.all(np.isfinite(got[:, LPD])), what
        _close(got[:, LPD], exp[:, LPD], RTOL, 1e-10 * A, what + ' LPD')


def _responses(model, rng, n):
    return 0.4 + rng.randn(n) if is_gauss(model) else (rng.rand(n) < 0.5).astype(np.float64)


# ------------------------------------------------------------------ (a) injected draws, every model family
ROWS = np.array([3, 0, 16, 17, 33])      # an empty site, a full tile, one row past a tile, three tiles


@pytest.mark.parametrize('model', ['m1b_sg', 'm2b_sg', 'm3b_sg', 'm4b_sg', 'm5b_sg', 'm1a_sg', 'm4a_sg'])
@pytest.mark.parametrize('D,S', [(1, 21), (3, 16), (21, 100), (32, 400), (128, 33)])
def test_injected_draws_match_the_host_prediction(model, D, S):
    K = 5
    X, y, k_lim, _, _, d, P = _site_problem(model, D, 7, 300 + D, K=K)
    eng = HipEngine(model, X, y, k_lim)
    assert eng.P == P
    rng = np.random.RandomState(7 + D)
    theta = 0.5 * rng.randn(K, S, P) + 0.3
    lim = np.concatenate(([0], np.cumsum(ROWS)))
    n = int(lim[-1])
    Xn, yn = 1.5 * rng.randn(n, D), _responses(model, rng, n)
    got = eng.predict(Xn, lim, y=yn, theta=theta)
    assert got.shape == (n, 4)
    for k in range(K):
        sl = slice(lim[k], lim[k + 1])
        _assert_site(model, D, 1, theta[k], Xn[sl], None, yn[sl], got[sl], 'site %d' % k)
    if is_gauss(model):
        assert got[:, MEAN].tobytes() == got[:, F_MEAN].tobytes()
    else:
        assert np.all((got[:, MEAN] > 0) & (got[:, MEAN] < 1))
    bare = eng.predict(Xn, lim, theta=theta)                            # without responses: no LPD, the rest unchanged
    assert np.all(np.isnan(bare[:, LPD])) and bare[:, :3].tobytes() == got[:, :3].tobytes()
    sub = eng.predict(Xn[lim[1]:lim[4]], lim[1:5] - lim[1], y=yn[lim[1]:lim[4]], k0=1, count=3, theta=theta[1:4])
    assert sub.tobytes() == got[lim[1]:lim[4]].tobytes()                # a sub-range: the same rows, the same bits
    eng.close()


# ------------------------------------------------------------------ (b) sites with several groups
@pytest.mark.parametrize('model,D,groups', [('m4b', 3, [[9], [8, 7, 9], [10, 6]]), ('m1b', 3, [[9], [8, 7, 9], [10, 6]]),
                                            ('m4b', 21, [[5], [4, 3, 4, 5, 3, 4]])])
def test_multi_group_sites_own_coordinates_and_row_order(model, D, groups):
    S, K = 30, len(groups)
    X, y, k_lim, g_cnt, g_lim, _, _, d = _group_problem(model, D, groups, 23)
    eng = HipEngine(model, X, y, k_lim, g_cnt=g_cnt, g_lim=g_lim)
    rng = np.random.RandomState(3)
    theta = np.full((K, S, eng.P), np.nan)                              # NaN behind every site's own coordinates
    for k in range(K):
        theta[k, :, :eng.site_P[k]] = 0.5 * rng.randn(S, eng.site_P[k]) + 0.3
    # new rows: 20 (more than a tile) in every site's first group, 3 in the others, none in the last group of all
    per_group = [[20] + [3] * (len(g) - 1) for g in groups]
    per_group[-1][-1] = 0
    cnt = np.array([sum(p) for p in per_group])
    lim = np.concatenate(([0], np.cumsum(cnt)))
    n = int(lim[-1])
    group = np.concatenate([np.repeat(np.arange(len(p)), p) for p in per_group]).astype(np.int32)
    Xn, yn = 1.2 * rng.randn(n, D), _responses(model, rng, n)
    got = eng.predict(Xn, lim, row_group=group, y=yn, theta=theta)      # rows in group order
    for k in range(K):
        sl = slice(lim[k], lim[k + 1])
        _assert_site(model, D, int(g_cnt[k]), theta[k, :, :eng.site_P[k]], Xn[sl], group[sl], yn[sl], got[sl],
                     'in order, site %d' % k)
    mix = np.concatenate([lim[k] + rng.permutation(cnt[k]) for k in range(K)])      # the groups of a site mixed
    got2 = eng.predict(Xn[mix], lim, row_group=group[mix], y=yn[mix], theta=theta)
    for k in range(K):
        sl = slice(lim[k], lim[k + 1])
        _assert_site(model, D, int(g_cnt[k]), theta[k, :, :eng.site_P[k]], Xn[mix][sl], group[mix][sl], yn[mix][sl],
                     got2[sl], 'mixed, site %d' % k)
    eng.close()


# ------------------------------------------------------------------ (c) saturated logits
def test_saturated_logits_give_exact_means_and_a_finite_lpd():
    D, K, S = 2, 2, 21
    X, y, k_lim, _, _, d, P = _site_problem('m1b_sg', D, 7, 5, K=K)
    eng = HipEngine('m1b_sg', X, y, k_lim)
    theta = np.zeros((K, S, P))                                         # [log sigma_a = 0, beta = 0 | eta]: f = eta
    theta[0, :, -1], theta[1, :, -1] = 750.0, -750.0
    Xn = np.random.RandomState(1).randn(6, D)
    yn = np.array([1.0, 0.0, 1.0, 1.0, 0.0, 1.0])
    got = eng.predict(Xn, [0, 3, 6], y=yn, theta=theta)
    print(got)
    assert np.all(got[:3, MEAN] == 1.0) and np.all(got[3:, MEAN] == 0.0)
    assert np.all(got[:3, F_MEAN] == 750.0) and np.all(got[3:, F_MEAN] == -750.0) and np.all(got[:, F_M2] == 0.0)
    wrong = np.array([1, 3, 5])                                         # y = 0 at f = 750, y = 1 at f = -750
    assert np.all(np.isfinite(got[:, LPD]))
    np.testing.assert_allclose(got[wrong, LPD], -750.0, rtol=RTOL)
    np.testing.assert_allclose(got[[0, 2, 4], LPD], 0.0, atol=1e-300)
    eng.close()


# ------------------------------------------------------------------ (d) linear predictors far from zero: centred sums
@pytest.mark.parametrize('S', [21, 400])
def test_ill_conditioned_predictors_need_the_centred_sum(S):
    D, K = 3, 2
    X, y, k_lim, _, _, d, P = _site_problem('m4a_sg', D, 7, 17, K=K)
    eng = HipEngine('m4a_sg', X, y, k_lim)
    rng = np.random.RandomState(S)
    theta = 0.5 * rng.randn(K, S, P)
    theta[:, :, 1] = 1e3 + 1e-2 * rng.randn(K, S)                       # mu_a (behind the family's log sigma)
    lim = np.array([0, 17, 20])
    Xn = rng.randn(20, D)
    yn = 1e3 + rng.randn(20)
    got = eng.predict(Xn, lim, y=yn, theta=theta)
    for k in range(K):
        sl = slice(lim[k], lim[k + 1])
        exp = site_params.predict_host(3, D, 1, True, theta[k], Xn[sl], None, yn[sl])
        print('S=%d site %d: F_M2 rel err %.3e' % (S, k, np.abs(got[sl, F_M2] / exp[:, F_M2] - 1).max()))
        np.testing.assert_allclose(got[sl, F_M2], exp[:, F_M2], rtol=RTOL)
        _assert_site('m4a_sg', D, 1, theta[k], Xn[sl], None, yn[sl], got[sl], 'site %d' % k)
    eng.close()


# ------------------------------------------------------------------ (e) the sampler's own draws, repeatability
def test_sampler_draws_on_the_device_and_repeatability():
    D, K = 4, 6
    X, y, k_lim, Oms, mus, d, P = _site_problem('m4b_sg', D, 40, 41, K=K, tight=4.0)
    eng, _, _ = _engine_with_cavity('m4b_sg', X, y, k_lim, Oms, mus)
    rng = np.random.RandomState(2)
    cnt = np.array([4, 17, 0, 1, 33, 2])
    lim = np.concatenate(([0], np.cumsum(cnt)))
    n = int(lim[-1])
    Xn, yn = rng.randn(n, D), (rng.rand(n) < 0.5).astype(np.float64)
    with pytest.raises(_lib.EpxError, match='no draws yet'):            # nothing sampled yet
        eng.predict(Xn, lim, y=yn)
    assert b'no draws yet' in eng.lib.epx_last_error()
    opts = HipEngine.sampler_opts(chains=4, iter=24, warmup=None, init='random')
    eng.sample_batch(np.arange(11, 11 + K, dtype=np.int64), opts)
    got = eng.predict(Xn, lim, y=yn)
    assert got.tobytes() == eng.predict(Xn, lim, y=yn).tobytes()        # twice: the same bits
    draws = np.stack([np.ascontiguousarray(eng.get_draws(k, all_params=True)) for k in range(K)])
    assert draws.shape == (K, 48, P)
    assert got.tobytes() == eng.predict(Xn, lim, y=yn, theta=draws).tobytes()
    for k in range(K):
        sl = slice(lim[k], lim[k + 1])
        _assert_site('m4b_sg', D, 1, draws[k], Xn[sl], None, yn[sl], got[sl], 'site %d' % k)
    sub = eng.predict(Xn[lim[2]:lim[5]], lim[2:6] - lim[2], y=yn[lim[2]:lim[5]], k0=2, count=3)
    assert sub.tobytes() == got[lim[2]:lim[5]].tobytes()                # a sub-range of the device draws
    eng.sample_batch(np.array([5, 6], dtype=np.int64), opts, k0=1, count=2)     # only sites 1, 2 are current now
    eng.predict(Xn[lim[1]:lim[3]], lim[1:4] - lim[1], k0=1, count=2)
    with pytest.raises(_lib.EpxError, match='left draws of sites'):
        eng.predict(Xn, lim, y=yn)
    eng.close()


# ------------------------------------------------------------------ (f) errors, not faults
def test_bad_arguments_are_errors():
    D, S = 3, 8
    X, y, k_lim, g_cnt, g_lim, _, _, d = _group_problem('m4b', D, [[9], [8, 7, 9], [10, 6]], 23)
    eng = HipEngine('m4b', X, y, k_lim, g_cnt=g_cnt, g_lim=g_lim)
    theta = np.zeros((3, S, eng.P))
    Xn, yn = np.ones((6, D)), np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0])
    lim = np.array([0, 1, 4, 6])
    group = np.array([0, 2, 0, 1, 1, 0], dtype=np.int32)
    assert eng.predict(Xn, lim, row_group=group, y=yn, theta=theta).shape == (6, 4)
    with pytest.raises(_lib.EpxError, match='row 1: group 3 outside'):
        eng.predict(Xn, lim, row_group=np.array([0, 3, 0, 1, 1, 0]), y=yn, theta=theta)
    with pytest.raises(_lib.EpxError, match='row 5: group 2 outside the 2 group'):
        eng.predict(Xn, lim, row_group=np.array([0, 2, 0, 1, 1, 2]), y=yn, theta=theta)
    with pytest.raises(_lib.EpxError, match='row 0: group -1 outside'):
        eng.predict(Xn, lim, row_group=np.array([-1, 2, 0, 1, 1, 0]), y=yn, theta=theta)
    with pytest.raises(_lib.EpxError, match='row 3: y = 0.5'):
        eng.predict(Xn, lim, row_group=group, y=np.where(np.arange(6) == 3, 0.5, yn), theta=theta)
    with pytest.raises(_lib.EpxError, match='row 2: y = nan'):
        eng.predict(Xn, lim, row_group=group, y=np.where(np.arange(6) == 2, np.nan, yn), theta=theta)
    with pytest.raises(_lib.EpxError, match='non-decreasing'):
        eng.predict(Xn, np.array([0, 7, 4, 6]), row_group=group, y=yn, theta=theta)
    with pytest.raises(_lib.EpxError, match='start at 0'):
        eng.predict(Xn, np.array([1, 2, 4, 6]), row_group=group, y=yn, theta=theta)
    for k0, count in ((-1, 2), (2, 2), (0, 0), (3, 1)):
        with pytest.raises(_lib.EpxError, match='site range'):
            eng.predict(Xn[:0], np.zeros(count + 1, dtype=np.int64), k0=k0, count=count, theta=theta[:max(count, 0)])
    out = np.full((1, 4), 7.0)                                          # n = 0: nothing launched, nothing written
    ns = ctypes.c_int()
    lim0 = np.zeros(4, dtype=np.int64)
    _lib.check(eng.lib.epx_predict(eng.ctx, 0, 3, lim0.ctypes.data_as(_lib.c_int64_p), None, None, None,
                                   _lib.dptr(theta), S, _lib.dptr(out), ctypes.byref(ns)))
    assert ns.value == S and np.all(out == 7.0)
    eng.close()


# ------------------------------------------------------------------ (g) Master.predict on the device
@pytest.mark.parametrize('J,K', [(4, 4), (5, 3)])
def test_master_predict_on_the_device(J, K):
    D = 3
    conf = fit.configurations(J=J, D=D, K=K, npg=30, siter=40, run_ep=True, damp=0.4)
    M = fit.main('m4b', conf, ret_master=True)
    assert isinstance(M.engine, HipEngine)
    assert M.run(2, verbose=False, calc_moments=False, seed=5) == 0
    multi = not M.model_name.endswith('_sg')
    assert multi == (K < J)
    j_ind = np.asarray(M.A_n['j_ind']) if multi else None
    res = M.predict(M.X, site_sizes=M.Nk, j_ind=j_ind, y_new=M.y)
    S = M.engine.num_draws()
    assert res['n'] == S and res['mean'].shape == (M.N,)
    assert np.all((res['mean'] > 0) & (res['mean'] < 1)) and np.all(res['f_var'] > 0)
    got = np.stack([res['mean'], res['f_mean'], res['f_var'] * (S - 1), res['lpd']], axis=1)
    yf = M.y.astype(np.float64)
    for k in range(K):
        sl = slice(M.k_lim[k], M.k_lim[k + 1])
        theta_k = M.engine.get_draws(k, all_params=True)
        theta_k = theta_k[:, :M.engine.site_P[k]] if multi else theta_k
        _assert_site(M.model_name, D, int(M._site_ng[k]), theta_k, M.X[sl], j_ind[sl] - 1 if multi else None, yf[sl],
                     got[sl], 'site %d' % k)
    shuffle = np.random.RandomState(0).permutation(M.N)                 # any order of the rows, by site index
    res2 = M.predict(M.X[shuffle], site_ind=np.asarray(M.k_ind)[shuffle], j_ind=j_ind[shuffle] if multi else None,
                     y_new=M.y[shuffle])
    for key in ('mean', 'f_mean', 'f_var', 'lpd'):
        np.testing.assert_allclose(res2[key], res[key][shuffle], rtol=1e-12, atol=1e-14)
