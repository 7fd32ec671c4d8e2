"""k_ppc / k_ppc_sites / epx_ppc / Master.ppc on the device: posterior predictive checks from draws in device memory,
against ppc.ppc_host (NumPy) on the same inputs.  Need a real MI355X.

Tolerances (derived, not tuned):
  - Bernoulli family, the integers.  A replicate is u1 < sigmoid(f): host and device use the same u1 (the stream is
    counter-based and bit-exact) and differ in sigmoid(f) by at most 1/4 of test_gpu_predict's bound on f,
    129 2^-53 A_i / 4, plus the absolute error of the lean logistic term pinned in test_gpu_lean_math.py (G_ABS).  The
    test asserts ON THE HOST, for its fixed seeds, that no cell's margin |u1 - sigmoid(f)| lies inside that bound -- a
    condition on the inputs (about 1e-9 likely to fail per case), not a tolerance -- and then T_MEAN, T_GE, T_GT and the
    exported T_rep_s have to equal the host's bit for bit; T_M2 at rtol 4 S 2^-53 (exact integers, only the centred sum
    rounds).  D_LE likewise: every |D_rep_s - D_obs_s| outside the two sums' bounds, exact ties (y_rep = y on every row)
    apart, which count on both sides.
  - D_obs_s, D_rep_s and everything of the Gaussian family: test_gpu_predict's per-term bounds added over the rows of
    the group -- rtol 1e-9 + atol 1e-10 max(1, A_i) per log-likelihood term, rtol 1e-9 + atol 1e-12 max(1, A_i) per f.
    The Gaussian replicate f + sigma z adds the device's exp, log, sqrt and sincos: the host statement is evaluated in
    float64 and in np.longdouble and the device may differ from the float64 host by 100 x their largest difference over
    the case, floored at 1e-12 relative (test_gpu_loo.py's rule).  Means over draws add the mean of the per-draw bounds
    and 4 S 2^-53 relative; T_M2 of real values adds 2 sum |T_s - mean| (e_s + mean e).  A count of the Gaussian family
    may differ by the number of draws whose comparison lies inside its bound.
Measured on an MI355X (largest error / bound over all cases): 6.0e-2 (T_OBS of a Gaussian group), 4.9e-2 for the centred
T_M2 of integers, below 1.3e-6 for every per-draw value and every mean of D; the Bernoulli integers equal the host's in
every case."""

import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from epstan_amd import _lib, fit, ppc                           # noqa: E402
from epstan_amd.draw_queries import CHECKS, HostDraws           # noqa: E402
from epstan_amd.engine import HipEngine, MODEL_IDS, is_gauss    # noqa: E402
from test_gpu_lean_math import G_ABS                             # noqa: E402
from test_gpu_parity import _site_problem, _group_problem       # noqa: E402
from test_gpu_predict import _scale, RTOL                        # noqa: E402

LD = np.longdouble
EPS = 2.0 ** -53
F_BOUND = 129 * EPS                       # |df| <= 129 2^-53 A_i (test_gpu_predict.py)
C = ppc.PC_COUNT
T_REP, D_OBS, D_REP = ppc.PD_T_REP, ppc.PD_D_OBS, ppc.PD_D_REP
WORST = {}


def _spec(model):
    return MODEL_IDS[model] % 5, is_gauss(model)


class Expect(object):
    """The host's records of a call and the error the device is allowed in every per-draw value."""


def _expect(model, D, site_ng, thetas, X, y, k_lim, group, seed, row0):
    """ppc_host on the inputs of a call, the bound e (G, 3, S) on every per-draw value, and -- Bernoulli family -- the
    conditions on the inputs under which the integers are exact, asserted here.  thetas[k]: (S, the site's own
    coordinates); group (N): 0-based group within the site, or None."""
    mid, gauss = _spec(model)
    ex = Expect()
    yf = np.asarray(y, dtype=np.float64)
    ex.groups, ex.sites, ex.draws = ppc.ppc_host(mid, D, site_ng, gauss, thetas, X, group, yf, k_lim, seed, row0)
    G, S = ex.draws.shape[0], ex.draws.shape[2]
    wide = None
    if gauss:
        with np.errstate(all='ignore'):
            wide = ppc.ppc_host(mid, D, site_ng, gauss, thetas, X, group, yf, k_lim, seed, row0, dtype=LD)[2]
        ref = np.abs((ex.draws - wide).astype(np.float64)).reshape(G, 3, S).max(axis=(0, 2))      # per value kind
    ex.e = np.zeros((G, 3, S))
    ex.tie = np.zeros((G, S), dtype=bool)
    ex.t_bound = np.zeros(G)
    ex.site_ng, ex.gauss, ex.S = np.asarray(site_ng), gauss, S
    gi = 0
    for k, ng in enumerate(site_ng):
        lo, hi = int(k_lim[k]), int(k_lim[k + 1])
        grp = np.zeros(hi - lo, dtype=np.int64) if group is None else np.asarray(group[lo:hi])
        rows = row0 + np.arange(lo, hi, dtype=np.int64)
        f, y_rep, ll_obs, ll_rep = ppc.site_cells(mid, D, ng, gauss, thetas[k], X[lo:hi], grp, yf[lo:hi], seed, rows)
        A = np.maximum(1.0, _scale(model, D, ng, thetas[k], X[lo:hi], grp))                # (n)
        if not gauss:
            margin = np.abs(ppc.replicate_uniforms(seed, rows, S) - ppc.sigmoid(f))
            inside = margin <= (0.25 * F_BOUND * A + G_ABS)[None, :]
            assert not inside.any(), 'site %d: %d cells decide their replicate inside the bound: take another seed' \
                % (k, inside.sum())
        for g in range(ng):
            at = np.nonzero(grp == g)[0]
            ex.e[gi, T_REP] = (RTOL * np.abs(f[:, at]) + 1e-12 * A[at]).sum(axis=1) if gauss else 0.0
            ex.e[gi, D_OBS] = (RTOL * np.abs(ll_obs[:, at]) + 1e-10 * A[at]).sum(axis=1)
            ex.e[gi, D_REP] = (RTOL * np.abs(ll_rep[:, at]) + 1e-10 * A[at]).sum(axis=1)
            ex.tie[gi] = np.all(y_rep[:, at] == yf[lo:hi][at][None, :], axis=1)
            ex.t_bound[gi] = 2 * at.size * EPS * np.abs(yf[lo:hi][at]).sum()       # two orders of adding up n responses
            gi += 1
    if gauss:
        ex.e += np.maximum(100.0 * ref[None, :, None], 1e-12 * np.abs(ex.draws))
    else:
        gap = np.abs(ex.draws[:, D_REP] - ex.draws[:, D_OBS])
        near = ~ex.tie & (gap <= ex.e[:, D_OBS] + ex.e[:, D_REP])
        assert not near.any(), '%d (group, draw) pairs compare D inside the bound: take another seed' % near.sum()
        assert np.all(ex.draws[:, D_REP][ex.tie] == ex.draws[:, D_OBS][ex.tie])
    return ex


def _site_values(ex, per_draw, err):
    """A site's per-draw values and bounds from its groups': added in group order."""
    first = np.concatenate(([0], np.cumsum(ex.site_ng)))
    v = np.stack([per_draw[first[k]:first[k + 1]].sum(axis=0) for k in range(len(ex.site_ng))])
    e = np.stack([err[first[k]:first[k + 1]].sum(axis=0) for k in range(len(ex.site_ng))])
    t_bound = np.add.reduceat(ex.t_bound, first[:-1])
    add = 4 * EPS * ex.site_ng.max()                        # adding the groups' values up, in another order on the host
    return v, e + add * np.abs(v), t_bound + add * np.abs(ex.sites[:, ppc.PC_T_OBS])


def _check_records(ex, got, host, v, e, t_bound, what):
    """Records `got` (U, 8) of U units against the host's, from the units' host per-draw values v (U, 3, S), their
    bounds e and the bound of T_obs; returns the largest error / bound."""
    S, worst = ex.S, 0.0
    assert got.shape == host.shape and not np.any(np.isnan(got)), what

    def close(col, bound, name):
        nonlocal worst
        err = np.abs(got[:, col] - host[:, col])
        ratio = float((err / np.maximum(bound, 1e-300)).max()) if np.any(err > 0) else 0.0
        print('%s %s: largest error %.3e, largest error / bound %.3e' % (what, name, err.max(), ratio))
        assert np.all(err <= bound), '%s %s' % (what, name)
        worst = max(worst, ratio)

    mean_e = e.mean(axis=2) + 4 * S * EPS * np.abs(v).mean(axis=2)                          # (U, 3)
    centred = np.abs(v[:, T_REP] - host[:, ppc.PC_T_MEAN][:, None])
    if ex.gauss:
        close(ppc.PC_T_OBS, t_bound, 'T_OBS')
        close(ppc.PC_T_MEAN, mean_e[:, T_REP], 'T_MEAN')
        close(ppc.PC_T_M2, 2 * (centred * (e[:, T_REP] + mean_e[:, T_REP][:, None])).sum(axis=1)
              + 4 * S * EPS * host[:, ppc.PC_T_M2], 'T_M2')
        t_obs = host[:, ppc.PC_T_OBS][:, None]
        near_t = (np.abs(v[:, T_REP] - t_obs) <= e[:, T_REP] + t_bound[:, None]).sum(axis=1)
        near_d = (np.abs(v[:, D_REP] - v[:, D_OBS]) <= e[:, D_REP] + e[:, D_OBS]).sum(axis=1)
        for col, near, name in ((ppc.PC_T_GE, near_t, 'T_GE'), (ppc.PC_T_GT, near_t, 'T_GT'), (ppc.PC_D_LE, near_d, 'D_LE')):
            assert np.all(np.abs(got[:, col] - host[:, col]) <= near), '%s %s' % (what, name)
            assert np.all(got[:, col] == np.rint(got[:, col])), what
    else:
        for col, name in ((ppc.PC_T_OBS, 'T_OBS'), (ppc.PC_T_MEAN, 'T_MEAN'), (ppc.PC_T_GE, 'T_GE'), (ppc.PC_T_GT, 'T_GT'),
                          (ppc.PC_D_LE, 'D_LE')):
            assert got[:, col].tobytes() == host[:, col].tobytes(), '%s %s: the integers are exact' % (what, name)
        close(ppc.PC_T_M2, 4 * S * EPS * host[:, ppc.PC_T_M2], 'T_M2')
    close(ppc.PC_D_OBS_MEAN, mean_e[:, D_OBS], 'D_OBS_MEAN')
    close(ppc.PC_D_REP_MEAN, mean_e[:, D_REP], 'D_REP_MEAN')
    return worst


def _compare(ex, groups, sites, draws, what):
    """Everything a call returned against the host; returns the largest error / bound."""
    G, S = ex.draws.shape[0], ex.S
    assert groups.shape == (G, C) and sites.shape == (len(ex.site_ng), C) and draws.shape == (G, 3, S), what
    if not ex.gauss:
        assert draws[:, T_REP].tobytes() == ex.draws[:, T_REP].tobytes(), what + ': T_rep_s are exact'
        assert np.all(draws[:, D_REP][ex.tie] == draws[:, D_OBS][ex.tie]), what + ': a tie is exact'
    err = np.abs(draws - ex.draws)
    assert np.all(err <= ex.e), what + ': per-draw values'
    worst = float((err / np.maximum(ex.e, 1e-300)).max())
    print('%s per-draw values: largest error %.3e, largest error / bound %.3e' % (what, err.max(), worst))
    worst = max(worst, _check_records(ex, groups, ex.groups, ex.draws, ex.e, ex.t_bound, what + ' groups'))
    sv, se, st = _site_values(ex, ex.draws, ex.e)
    worst = max(worst, _check_records(ex, sites, ex.sites, sv, se, st, what + ' sites'))
    single = np.all(ex.site_ng == 1)
    if single:
        assert sites.tobytes() == groups.tobytes(), what + ': the site repeats its one group'
    WORST[what] = worst
    return worst


# ------------------------------------------------------------------ (a) shapes at the edges of the walk
SIZES = [[1, 16], [17, 64, 65], [5]]                        # a tile and its edges, the second item of a group; unequal


def _problem(model, D, S, seed, sizes=SIZES):
    """(engine, X, y, k_lim, site_ng, group, theta (K, S, P), thetas): the sites hold the groups `sizes`; an `_sg` model
    gets one site per group."""
    if model.endswith('_sg'):
        sizes = [[n] for s in sizes for n in s]
    X, y, k_lim, g_cnt, g_lim, _, _, d = _group_problem(model, D, sizes, seed)
    multi = not model.endswith('_sg')
    eng = HipEngine(model, X, y, k_lim, **(dict(g_cnt=g_cnt, g_lim=g_lim) if multi else {}))
    K = len(sizes)
    rng = np.random.RandomState(seed + 1)
    site_P = eng.site_P if multi else np.full(K, eng.P)
    theta = np.full((K, S, eng.P), np.nan)                  # NaN behind every site's own coordinates
    for k in range(K):
        theta[k, :, :site_P[k]] = 0.5 * rng.randn(S, site_P[k]) + 0.3
    thetas = [theta[k, :, :site_P[k]] for k in range(K)]
    group = np.concatenate([np.repeat(np.arange(len(s)), s) for s in sizes]) if multi else None
    return eng, X, y, k_lim, [len(s) for s in sizes], group, theta, thetas


@pytest.mark.parametrize('model', ['m1b_sg', 'm4b', 'm5b', 'm4a'])
@pytest.mark.parametrize('D,S', [(1, 17), (3, 32), (4, 33)])
def test_injected_draws_match_the_host_checks(model, D, S):
    eng, X, y, k_lim, site_ng, group, theta, thetas = _problem(model, D, S, 70 + D)
    N = int(k_lim[-1])
    seed, row0 = 1000 + S, {1: 0, 3: 7, 4: 2 ** 32 - N - 1}[D]       # (the last: rows beyond 2^31, up to the limit)
    ex = _expect(model, D, site_ng, thetas, X, y, k_lim, group, seed, row0)
    groups, sites, draws, n = eng.replicated_checks(seed=seed, row0=row0, theta=theta, with_n=True, with_draws=True)
    assert n == S
    _compare(ex, groups, sites, draws, '%s D=%d S=%d' % (model, D, S))
    eng.close()


def test_a_workgroup_walks_its_groups():
    """More groups than the grid holds workgroups (1024 on 256 compute units): a workgroup starts its next group from
    zeroed sums and a cleared flag -- the NaN planted in site 3 stays there -- and the site stage takes many blocks."""
    K, n, D, S = 1100, 2, 1, 17
    X, y, k_lim, _, _, d, P = _site_problem('m1b_sg', D, n, 9, K=K)
    eng = HipEngine('m1b_sg', X, y, k_lim)
    theta = 0.5 * np.random.RandomState(4).randn(K, S, P) + 0.3
    ex = _expect('m1b_sg', D, [1] * K, list(theta), X, y, k_lim, None, 21, 0)
    groups, sites, draws = eng.replicated_checks(seed=21, theta=theta, with_draws=True)
    _compare(ex, groups, sites, draws, '1100 groups')
    assert ex.tie.any()                                     # two rows: some draws replicate the data
    theta[3, 5, 0] = np.nan
    bad, bad_sites = eng.replicated_checks(seed=21, theta=theta)
    hit = np.arange(K) == 3
    assert np.all(np.isnan(bad[hit])) and bad[~hit].tobytes() == groups[~hit].tobytes()
    assert bad_sites.tobytes() == bad.tobytes()
    eng.close()


# ------------------------------------------------------------------ (b) the same bits
@pytest.mark.parametrize('model', ['m4b', 'm4a'])
def test_same_bits_whatever_the_call(model):
    D, S = 3, 33
    eng, X, y, k_lim, site_ng, group, theta, thetas = _problem(model, D, S, 5)
    K = len(site_ng)
    one = eng.replicated_checks(seed=8, row0=11, theta=theta, with_draws=True)
    two = eng.replicated_checks(seed=8, row0=11, theta=theta, with_draws=True)
    for a, b in zip(one, two):
        assert a.tobytes() == b.tobytes()                   # twice: the same bytes
    # a replicate is a function of (seed, row, draw): the sites [0, K) equal [0, 1) and [1, K) side by side -- the
    # context's rows keep their index, so the matching row0 is the same one
    head = eng.replicated_checks(seed=8, row0=11, k0=0, count=1, theta=theta[:1], with_draws=True)
    tail = eng.replicated_checks(seed=8, row0=11, k0=1, count=K - 1, theta=theta[1:], with_draws=True)
    for a, h, t in zip(one, head, tail):
        assert a.tobytes() == np.concatenate((h, t)).tobytes()
    other = eng.replicated_checks(seed=9, row0=11, theta=theta, with_draws=True)
    assert np.any(other[2][:, T_REP] != one[2][:, T_REP])
    moved = eng.replicated_checks(seed=8, row0=12, theta=theta, with_draws=True)
    assert np.any(moved[2][:, T_REP] != one[2][:, T_REP])
    assert moved[2][:, D_OBS].tobytes() == one[2][:, D_OBS].tobytes()       # the observed side does not see the stream
    eng.close()


# ------------------------------------------------------------------ (c) NaN
@pytest.mark.parametrize('model', ['m4b', 'm4a'])
def test_a_nan_draw_makes_its_site_nan_and_no_other(model):
    D, S = 3, 20
    eng, X, y, k_lim, site_ng, group, theta, thetas = _problem(model, D, S, 6)
    good_g, good_s = eng.replicated_checks(seed=2, theta=theta)
    assert np.all(np.isfinite(good_g)) and np.all(np.isfinite(good_s))
    kept = theta[1, 13, 0]
    theta[1, 13, 0] = np.nan                                # phi[0] of one draw of site 1: every group of the site reads it
    got_g, got_s = eng.replicated_checks(seed=2, theta=theta)
    first = np.concatenate(([0], np.cumsum(site_ng)))
    hit = np.zeros(first[-1], dtype=bool)
    hit[first[1]:first[2]] = True
    assert np.all(np.isnan(got_g[hit])) and got_g[~hit].tobytes() == good_g[~hit].tobytes()
    assert np.all(np.isnan(got_s[1])) and got_s[[0, 2]].tobytes() == good_s[[0, 2]].tobytes()
    theta[1, 13, 0] = kept
    d = eng.d
    theta[1, 2, d + 1] = np.inf                             # eta of group 1 of site 1 alone: its group, and the site
    got_g, got_s = eng.replicated_checks(seed=2, theta=theta)
    hit[:] = False
    hit[first[1] + 1] = True
    assert np.all(np.isnan(got_g[hit])) and got_g[~hit].tobytes() == good_g[~hit].tobytes()
    assert np.all(np.isnan(got_s[1])) and got_s[[0, 2]].tobytes() == good_s[[0, 2]].tobytes()
    eng.close()


# ------------------------------------------------------------------ (d) refusals
def _raw(eng, k0, count, seed, row0, theta, S, groups, sites=None, draws=None):
    import ctypes
    return eng.lib.epx_ppc(eng.ctx, k0, count, ctypes.c_uint64(seed), row0, _lib.dptr(theta), S, _lib.dptr(groups),
                           _lib.dptr(sites), _lib.dptr(draws), None)


def test_refusals_launch_nothing():
    D, K, n = 1, 2, 3
    X, y, k_lim, _, _, d, P = _site_problem('m1b_sg', D, n, 5, K=K)
    eng = HipEngine('m1b_sg', X, y, k_lim)
    groups, sites = np.full((K, C), 7.0), np.full((K, C), 7.0)
    small = np.zeros((K, 4, P))
    # S beyond the LDS: the limit is in the text (no copy has been queued: the S of this call is not read)
    assert _raw(eng, 0, K, 0, 0, small, 10 ** 7, groups, sites) != 0
    text = eng.lib.epx_last_error().decode()
    m = re.search(r'S = 10000000 draws, at most (\d+)', text)
    assert m, text
    limit = int(m.group(1))
    assert 6000 < limit < 6900                              # (160 KiB - 1 KiB - the fixed part) / 24 bytes at D = 1
    theta = 0.5 * np.random.RandomState(1).randn(K, limit + 1, P)
    with pytest.raises(_lib.EpxError, match=r'S = %d draws, at most %d' % (limit + 1, limit)):
        eng.replicated_checks(theta=theta)
    at_limit = np.ascontiguousarray(theta[:, :limit])
    ex = _expect('m1b_sg', D, [1] * K, list(at_limit), X, y, k_lim, None, 0, 0)
    _compare(ex, *eng.replicated_checks(theta=at_limit, with_draws=True), 'S at the LDS limit')
    # rows of the stream: row0 + rows has to stay below 2^32
    N = int(k_lim[-1])
    for row0 in (2 ** 32 - N, 2 ** 32, -1):
        assert _raw(eng, 0, K, 0, row0, small, 4, groups, sites) != 0
        assert b'row0' in eng.lib.epx_last_error()
    assert _raw(eng, 0, 1, 0, 2 ** 32 - n, small, 4, groups, sites) != 0 and b'row0' in eng.lib.epx_last_error()
    assert _raw(eng, 0, K, 0, 0, small, 4, None, sites) != 0 and b'out_groups' in eng.lib.epx_last_error()
    assert _raw(eng, 0, K, 0, 0, small, 0, groups, sites) != 0 and b'S = 0' in eng.lib.epx_last_error()
    with pytest.raises(_lib.EpxError, match='no draws yet'):
        eng.replicated_checks()
    for k0, count in ((-1, 2), (1, 2), (0, 0), (2, 1)):
        with pytest.raises(_lib.EpxError, match='site range'):
            eng.replicated_checks(k0=k0, count=count, theta=np.zeros((max(count, 0), 4, P)))
    assert np.all(groups == 7.0) and np.all(sites == 7.0)   # nothing was written
    assert _raw(eng, 0, K, 0, 2 ** 32 - N - 1, small, 4, groups, None) == 0 and np.all(np.isfinite(groups))   # sites may be NULL
    eng.close()
    D = 129                                                 # EPX_PR_DMAX = 128
    rng = np.random.RandomState(2)
    eng = HipEngine('m1b_sg', rng.randn(2, D), np.array([0, 1]), np.array([0, 2]))
    with pytest.raises(_lib.EpxError, match='D = 129 columns, at most 128'):
        eng.replicated_checks(theta=np.zeros((1, 4, eng.P)))
    eng.close()


# ------------------------------------------------------------------ (e) Master.ppc on the device
class _Spy(object):
    """Counts the calls of CHECKS that reach `target`."""

    def __init__(self, target):
        self.target, self.calls = target, []

    def __getattr__(self, name):
        if name not in CHECKS:
            raise AttributeError(name)
        self.calls.append(name)
        return getattr(self.target, name)


@pytest.mark.parametrize('J,K', [(4, 2), (3, 3)])
def test_master_ppc_on_the_device(J, K):
    """The device route `Master` takes as built against the host route forced over the same `HipEngine`: both read the
    same device draws (the pattern of test_gpu_draw_queries.py)."""
    D = 2
    conf = fit.configurations(J=J, D=D, K=K, npg=30, siter=40, chains=4, run_ep=True, damp=0.4)
    M = fit.main('m4b', conf, ret_master=True)
    assert isinstance(M.engine, HipEngine) and isinstance(M._queries.host, HostDraws)
    with pytest.raises(RuntimeError, match='before at least one iteration'):
        M.ppc()
    assert M.run(1, verbose=False, calc_moments=False, seed=5) == 0
    dev = M.ppc(seed=3, draws=True)
    resolver = M._queries
    spy = M._queries = _Spy(resolver.host)
    try:
        host = M.ppc(seed=3, draws=True)
    finally:
        M._queries = resolver
    assert spy.calls == ['replicated_checks']
    S = M.engine.num_draws()
    assert dev['n'] == host['n'] == S and dev['draws'].shape == (J, 3, S)
    multi = not M.model_name.endswith('_sg')
    assert multi == (K < J)
    raw = M.engine.replicated_checks(seed=3, row0=0, with_draws=True)
    again = ppc.summarise(raw[0], raw[1], S, M._site_ng, draws=raw[2])
    for key in dev:                                          # the dict is the summary of the engine's records
        assert np.asarray(dev[key]).tobytes() == np.asarray(again[key]).tobytes(), key
    thetas = [np.ascontiguousarray(M.engine.get_draws(k, all_params=True))[:, :M.engine.site_P[k] if multi else None]
              for k in range(K)]
    group = np.asarray(M.A_n['j_ind']) - 1 if multi else None
    ex = _expect(M.model_name, D, [int(g) for g in M._site_ng], thetas, M.X, M.y, M.k_lim, group, 3, 0)
    assert host['draws'].tobytes() == ex.draws.tobytes()     # the host route IS ppc_host on these draws
    _compare(ex, raw[0], raw[1], raw[2], 'Master J=%d K=%d' % (J, K))
    for key in ('group_site', 't_obs', 't_rep_mean', 'p_t_ge', 'p_t', 'p_d', 'site_t_obs', 'site_p_t', 'site_p_d', 'extreme'):
        assert np.asarray(dev[key]).tobytes() == np.asarray(host[key]).tobytes(), key        # the Bernoulli integers
    np.testing.assert_array_equal(dev['site_t_obs'], np.add.reduceat(M.y, M.k_lim[:-1]))


def test_zz_report():
    """The largest error / bound of every case above."""
    for what, worst in sorted(WORST.items()):
        print('%-40s largest error / bound %.3e' % (what, worst))
    if WORST:
        print('over all cases: %.3e' % max(WORST.values()))
