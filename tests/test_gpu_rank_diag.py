"""k_rank_diag / epx_draw_rank_diagnostics / epx_rank_normalize / Master.diagnostics(rank=True) on the device: the
rank-normalised split-Rhat, bulk-ESS and tail-ESS from draws in device memory, against diagnostics.rank_diagnostics_host
(NumPy, SciPy's ndtri) on the same draws.  Need a real MI355X.

Tolerance (derived, not tuned).  Ranks, med, q05, q95, |x - med| and the indicators are exact by construction: the device
and the host evaluate the same expressions on the same doubles, and epx_rank_normalize's ranks are compared with `==`.  From
there on the series go through the procedure of EPX_DG_ESS, whose bound test_gpu_draw_diag.py derives: rho(t) is a sum of
h <= 200 products and tau a sum of <= 100 pairs, so the error is <~ 2 10^4 2^-53 relative to tau >= 1 / log10(n) > 0.25:
rtol 1e-9 leaves two orders of margin (1e-8 for h > 200).  The one new source of error is Phi^-1: the device's normcdfinv
and SciPy's ndtri differ by a few ulp of a score |z| < 3.8, at most ZTOL = 7.2e-15 absolute (measured, below).  A
perturbation dz of the scores enters every centred product linearly, so rho(t) moves by <~ 2 dz max|z| / W =
2 7.2e-15 3.8 / 0.9 < 1e-13, summed over <= 100 pairs < 1e-11 relative to tau > 0.25: two orders inside the bound, which
carries over.  The stop rule is continuous: a pair that rounding moves across 0 contributes about 0."""

import numpy as np
import pytest
import scipy.special

pytestmark = pytest.mark.gpu

from epstan_amd import _lib, fit                              # noqa: E402
from epstan_amd.diagnostics import (RD_COUNT, RD_ESS_BULK, RD_ESS_TAIL, RD_MAX_DRAWS, RD_NAMES, RD_RHAT_BULK,   # noqa: E402
                                    rank_diagnostics_host, rank_normalize_host)
from epstan_amd.engine import HipEngine                       # noqa: E402
from test_gpu_parity import _site_problem, _group_problem     # noqa: E402
from test_gpu_draw_diag import ar1                            # noqa: E402

RTOL = 1e-9
# max |normcdfinv - ndtri| over the arguments (r - 3/8) / (n + 1/4), r = 1..n, n = 8 ... RD_MAX_DRAWS, measured on an
# MI355X: 1.8e-15 (test_normal_scores_against_ndtri); asserted at 4 x that for the spread of devices' math libraries, and
# never above 1e-12: adjacent ranks at n = 16384 are >= 1.5e-4 apart in z, anything near 1e-12 would still be rounding,
# anything above it a wrong formula
ZTOL = 7.2e-15


def _close(got, exp, rtol, what):
    assert got.shape == exp.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(exp)), what
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.abs(got - exp) / np.abs(exp)
    rel = np.where(np.isnan(exp) | (got == exp), 0.0, rel)
    print('%s: largest relative error per field %s' % (what, ' '.join('%.2e' % v for v in rel.reshape(-1, RD_COUNT).max(axis=0))))
    assert np.all(rel <= rtol), what


@pytest.fixture(scope='module')
def small():
    """One small engine for the tests that only need a device and a record stride: m4b_sg, D = 3, K = 3."""
    X, y, k_lim, _, _, d, P = _site_problem('m4b_sg', 3, 7, 5, K=3)
    eng = HipEngine('m4b_sg', X, y, k_lim)
    yield eng
    eng.close()


# ------------------------------------------------------------------ (a) the ranking stage alone
@pytest.mark.parametrize('n', [256, 258, 254, 8])
def test_ranks_are_exactly_the_hosts(small, n):
    rng = np.random.RandomState(n)
    zeros = rng.permutation(np.tile([0.0, -0.0, 1.5, -2.0], n // 4 + 1)[:n])          # +-0.0 tie; two more values
    x = np.stack([rng.randn(n), np.round(2 * rng.randn(n)) / 2, zeros, np.full(n, -3.25), np.arange(n, 0.0, -1.0),
                  np.where(np.arange(n) == n // 3, 7.0, 1.0)])
    assert np.signbit(zeros[zeros == 0]).any() and not np.signbit(zeros[zeros == 0]).all()
    for fold in (False, True):
        rank, z = small.rank_normalize(x, fold=fold)
        erank, ez = rank_normalize_host(x, fold=fold)
        np.testing.assert_array_equal(rank, erank)
        assert np.max(np.abs(z - ez)) <= ZTOL
        assert np.array_equal(z == 0.0, ez == 0.0)                      # the middle rank: exactly 0 on both sides
    rank, z = small.rank_normalize(x)
    np.testing.assert_array_equal(rank[3], np.full(n, (n + 1) / 2.0))   # a constant series: one run of n
    np.testing.assert_array_equal(rank[4], np.arange(n, 0.0, -1.0))
    bad = x.copy()
    bad[1, n // 2] = np.nan
    bad[4, 0] = -np.inf
    rank, z = small.rank_normalize(bad)
    assert np.all(np.isnan(rank[[1, 4]])) and np.all(np.isnan(z[[1, 4]]))
    np.testing.assert_array_equal(rank[[0, 2, 3, 5]], rank_normalize_host(x[[0, 2, 3, 5]])[0])    # that series alone


def test_normal_scores_against_ndtri(small):
    """Every argument (r - 3/8) / (n + 1/4), r = 1..n, at n = 8, 100, 800, 4096 and the limit 8140.  Measured on an
    MI355X: max |z_device - ndtri| = 2.2e-16, 6.7e-16, 8.9e-16, 1.3e-15 and 1.8e-15 (1.776e-15, at
    |z| = 3.785: four ulp); ZTOL is four times the largest."""
    worst = 0.0
    for n in (8, 100, 800, 4096, RD_MAX_DRAWS):
        x = np.random.RandomState(n).permutation(n).astype(np.float64)[None, :]
        rank, z = small.rank_normalize(x)
        np.testing.assert_array_equal(rank, x + 1.0)
        err = float(np.max(np.abs(z - scipy.special.ndtri((rank - 0.375) / (n + 0.25)))))
        print('n = %d: max |z - ndtri| = %.3e (largest |z| %.3f)' % (n, err, np.abs(z).max()))
        worst = max(worst, err)
    assert ZTOL <= 1e-12 and worst <= ZTOL


# ------------------------------------------------------------------ (b) injected draws
@pytest.mark.parametrize('model', ['m1b_sg', 'm4b_sg', 'm4a_sg'])
@pytest.mark.parametrize('D', [1, 3, 32])
@pytest.mark.parametrize('chains,nkeep', [(1, 4), (2, 5), (4, 9), (4, 32), (3, 401)])
def test_injected_draws_match_the_host(model, D, chains, nkeep):
    K = 3
    X, y, k_lim, _, _, d, P = _site_problem(model, D, 7, 300 + D, K=K)
    eng = HipEngine(model, X, y, k_lim)
    assert eng.P == P
    theta = ar1(np.random.RandomState(1000 * chains + nkeep + D), K, chains, nkeep, P)
    got, n = eng.draw_rank_diagnostics(theta=theta, chains=chains, with_n=True)
    assert got.shape == (K, P, RD_COUNT) and n == 2 * chains * (nkeep // 2)
    for k in range(K):
        _close(got[k], rank_diagnostics_host(theta[k], chains), RTOL, 'site %d' % k)          # (h <= 200)
    assert np.all(np.isfinite(got[:, :, [RD_RHAT_BULK, RD_ESS_BULK]])) and np.all(got[:, :, RD_ESS_BULK] > 0)
    assert got.tobytes() == eng.draw_rank_diagnostics(theta=theta, chains=chains).tobytes()    # twice: the same bits
    sub = eng.draw_rank_diagnostics(k0=1, count=2, theta=theta[1:3], chains=chains)
    assert sub.tobytes() == got[1:3].tobytes()                          # a sub-range: the same bits
    eng.close()


# ------------------------------------------------------------------ (c) ties
def test_tied_draws_match_the_host(small):
    chains, nkeep, K, P = 4, 50, small.K, small.P
    theta = np.round(2 * ar1(np.random.RandomState(6), K, chains, nkeep, P)) / 2          # about ten distinct values
    assert len(np.unique(theta[0, :, 1])) < 16
    theta[1, :, 2] = 1.25
    theta[1, 77, 2] = 3.0                                               # all but one draw equal, the odd one above ...
    theta[2, :, 4] = 1.25
    theta[2, 120, 4] = -3.0                                             # ... and below: x <= q05 holds for every draw
    got = small.draw_rank_diagnostics(theta=theta, chains=chains)
    for k in range(K):
        _close(got[k], rank_diagnostics_host(theta[k], chains), RTOL, 'site %d' % k)
    assert np.isfinite(got[1, 2, RD_ESS_TAIL]) and np.isnan(got[2, 4, RD_ESS_TAIL]) and np.isfinite(got[2, 4, RD_ESS_BULK])


# ------------------------------------------------------------------ (d) sites with several groups
@pytest.mark.parametrize('model,D,groups', [('m4b', 3, [[9], [8, 7, 9], [10, 6]]), ('m1b', 3, [[9], [8, 7, 9], [10, 6]])])
def test_multi_group_sites_nan_behind_their_own_coordinates(model, D, groups):
    chains, nkeep, K = 4, 24, len(groups)
    X, y, k_lim, g_cnt, g_lim, _, _, d = _group_problem(model, D, groups, 23)
    eng = HipEngine(model, X, y, k_lim, g_cnt=g_cnt, g_lim=g_lim)
    assert len(set(eng.site_P)) > 1
    draws = ar1(np.random.RandomState(3), K, chains, nkeep, eng.P)
    theta = np.full_like(draws, np.nan)                                 # NaN behind every site's own coordinates
    for k in range(K):
        theta[k, :, :eng.site_P[k]] = draws[k, :, :eng.site_P[k]]
    got = eng.draw_rank_diagnostics(theta=theta, chains=chains)
    for k in range(K):
        Pk = int(eng.site_P[k])
        assert np.all(np.isnan(got[k, Pk:])) and np.all(np.isfinite(got[k, :Pk, RD_ESS_BULK]))
        _close(got[k, :Pk], rank_diagnostics_host(theta[k, :, :Pk], chains), RTOL, 'site %d' % k)
    # what lies behind a site's coordinates plays no part
    assert np.array_equal(got, eng.draw_rank_diagnostics(theta=np.where(np.isnan(theta), 1e300, theta), chains=chains),
                          equal_nan=True)
    eng.close()


# ------------------------------------------------------------------ (e) results, never faults
def test_nan_inf_constant_and_short_chains_give_nan_not_faults(small):
    K, P, chains, nkeep = small.K, small.P, 4, 20
    theta = ar1(np.random.RandomState(4), K, chains, nkeep, P)
    ref = small.draw_rank_diagnostics(theta=theta, chains=chains)
    bad = theta.copy()
    bad[0, :, 1] = 2.5                                                  # a coordinate that never moved
    bad[0, 7, 3] = np.nan
    bad[1, 50, 4] = np.inf
    bad[2, 0, 0] = -np.inf
    got = small.draw_rank_diagnostics(theta=bad, chains=chains)
    hit = np.zeros((K, P), dtype=bool)
    hit[0, [1, 3]] = hit[1, 4] = hit[2, 0] = True
    assert np.all(np.isnan(got[hit]))
    assert got[~hit].tobytes() == ref[~hit].tobytes()                   # the other coordinates: untouched
    for k in range(K):
        _close(got[k], rank_diagnostics_host(bad[k], chains), RTOL, 'site %d' % k)
    for short in (3, 2, 1):                                             # fewer than 4 draws per chain
        got = small.draw_rank_diagnostics(theta=theta[:, :chains * short], chains=chains)
        assert got.shape == (K, P, RD_COUNT) and np.all(np.isnan(got))


# ------------------------------------------------------------------ (f) the limit on the used draws
def test_the_limit_on_used_draws():
    X, y, k_lim, _, _, d, P = _site_problem('m1b_sg', 1, 7, 9, K=1)
    eng = HipEngine('m1b_sg', X, y, k_lim)
    chains, nkeep = 2, RD_MAX_DRAWS // 4 * 2 + 1                        # odd: the middle draw is dropped
    theta = ar1(np.random.RandomState(8), 1, chains, nkeep, P)
    got, n = eng.draw_rank_diagnostics(theta=theta, chains=chains, with_n=True)
    assert n == RD_MAX_DRAWS == 8140
    _close(got[0], rank_diagnostics_host(theta[0], chains), 1e-8, 'n = %d' % n)
    assert got.tobytes() == eng.draw_rank_diagnostics(theta=theta, chains=chains).tobytes()
    more = np.random.RandomState(9).randn(1, RD_MAX_DRAWS + 2, P)
    with pytest.raises(_lib.EpxError, match='%d used draws per site, at most %d' % (RD_MAX_DRAWS + 2, RD_MAX_DRAWS)):
        eng.draw_rank_diagnostics(theta=more, chains=1)
    with pytest.raises(_lib.EpxError, match='at most %d' % RD_MAX_DRAWS):
        eng.rank_normalize(more[0, :, :1].T)
    with pytest.raises(_lib.EpxError, match='no multiple of chains'):   # the refusals of epx_draw_diagnostics, in its order
        eng.draw_rank_diagnostics(theta=more, chains=4)
    with pytest.raises(_lib.EpxError, match='no draws yet'):
        eng.draw_rank_diagnostics()
    eng.close()


# ------------------------------------------------------------------ (g) end to end
@pytest.mark.parametrize('J,K', [(4, 4), (5, 3)])
def test_master_rank_diagnostics_on_the_device(J, K):
    conf = fit.configurations(J=J, D=3, K=K, npg=30, siter=40, run_ep=True, damp=0.4)
    M = fit.main('m4b', conf, ret_master=True)
    assert isinstance(M.engine, HipEngine)
    assert M.run(1, verbose=False, calc_moments=False, seed=5) == 0
    plain, res = M.diagnostics(), M.diagnostics(rank=True)
    for key in plain:
        if key != 'worst':
            np.testing.assert_array_equal(res[key], plain[key])
    chains = M.workers[0].stan_params['chains']
    multi = not M.model_name.endswith('_sg')
    assert multi == (K < J)
    for k in range(K):
        Pk = int(M.engine.site_P[k]) if multi else M.engine.P
        exp = rank_diagnostics_host(np.ascontiguousarray(M.engine.get_draws(k, all_params=True))[:, :Pk], chains)
        got = np.stack([res[name][k] for name in RD_NAMES], axis=1)
        assert got.shape == (M.engine.P, RD_COUNT) and np.all(np.isnan(got[Pk:])) and np.all(np.isfinite(got[:Pk, RD_ESS_BULK]))
        _close(got[:Pk], exp, RTOL, 'site %d' % k)
    np.testing.assert_array_equal(res['site_max_rhat_rank'], np.nanmax(res['rhat_rank'], axis=1))
    np.testing.assert_array_equal(res['site_min_ess_rank'], np.nanmin(np.fmin(res['ess_bulk'], res['ess_tail']), axis=1))
    np.testing.assert_array_equal(res['rhat_rank'], np.maximum(res['rhat_bulk'], res['rhat_folded']))
