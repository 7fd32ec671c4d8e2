"""k_draw_diag / epx_draw_diagnostics / Master.diagnostics on the device: per-coordinate split-Rhat, effective sample
sizes and Monte-Carlo standard error from draws in device memory, against diagnostics.diagnostics_host (NumPy) on the
same draws.  Need a real MI355X.

Tolerance (derived, not tuned): rho(t) is a sum of h <= 200 products and tau a sum of <= 100 pairs, so the error is
<~ 2 10^4 2^-53 relative to tau >= 1 / log10(n) > 0.25: rtol 1e-9 leaves two orders of margin (1e-8 at h = 2500).  The
stop rule is continuous: a pair that rounding moves across 0 contributes about 0."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from epstan_amd import _lib, fit                              # noqa: E402
from epstan_amd.diagnostics import (DG_COUNT, DG_ESS, DG_ESS_SQ, DG_MCSE, DG_MEAN, DG_RHAT, DG_VAR,   # noqa: E402
                                    diagnostics_host)
from epstan_amd.engine import HipEngine                       # noqa: E402
from epstan_amd.method import Worker                          # noqa: E402
from test_gpu_parity import _site_problem, _engine_with_cavity, _group_problem   # noqa: E402

RTOL = 1e-9
NAN4 = [DG_RHAT, DG_ESS, DG_MCSE, DG_ESS_SQ]
PHIS = np.array([-0.5, 0.0, 0.5, 0.9, 0.99])


def ar1(rng, K, chains, nkeep, P):
    """(K, chains * nkeep, P) chain-major stationary AR(1) draws, coordinate e with phi = PHIS[e % 5] and its own
    level: neighbouring lanes stop at different lags."""
    phi = PHIS[np.arange(P) % 5]
    x = np.empty((K, chains, nkeep, P))
    x[:, :, 0] = rng.randn(K, chains, P) / np.sqrt(1 - phi ** 2)
    for t in range(1, nkeep):
        x[:, :, t] = phi * x[:, :, t - 1] + rng.randn(K, chains, P)
    return (x + 0.3 * rng.randn(P)).reshape(K, chains * nkeep, P)


def _close(got, exp, rtol, what):
    assert got.shape == exp.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(exp)), what
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.abs(got - exp) / np.abs(exp)
    rel = np.where(np.isnan(exp) | (got == exp), 0.0, rel)
    print('%s: largest relative error per field %s' % (what, ' '.join('%.2e' % v for v in rel.max(axis=0))))
    assert np.all(rel <= rtol), what


# ------------------------------------------------------------------ (a) injected draws
@pytest.mark.parametrize('model', ['m1b_sg', 'm4b_sg', 'm4a_sg'])
@pytest.mark.parametrize('D', [1, 3, 21, 32, 128])
@pytest.mark.parametrize('chains,nkeep', [(1, 4), (2, 5), (4, 9), (4, 24), (4, 100), (3, 401)])
def test_injected_draws_match_the_host_diagnostics(model, D, chains, nkeep):
    K = 5
    X, y, k_lim, _, _, d, P = _site_problem(model, D, 7, 300 + D, K=K)
    eng = HipEngine(model, X, y, k_lim)
    assert eng.P == P
    theta = ar1(np.random.RandomState(1000 * chains + nkeep + D), K, chains, nkeep, P)
    got, n = eng.draw_diagnostics(theta=theta, chains=chains, with_n=True)
    assert got.shape == (K, P, DG_COUNT) and n == 2 * chains * (nkeep // 2)
    for k in range(K):
        _close(got[k], diagnostics_host(theta[k], chains), RTOL, 'site %d' % k)
    assert np.all(np.isfinite(got)) and np.all(got[:, :, DG_ESS] > 0) and np.all(got[:, :, DG_ESS_SQ] > 0)
    assert got.tobytes() == eng.draw_diagnostics(theta=theta, chains=chains).tobytes()         # twice: the same bits
    sub = eng.draw_diagnostics(k0=1, count=3, theta=theta[1:4], chains=chains)
    assert sub.tobytes() == got[1:4].tobytes()                          # a sub-range: the same bits
    eng.close()


# ------------------------------------------------------------------ (b) a run beyond the LDS tile
def test_a_long_run_beyond_the_lds_tile():
    chains, nkeep, D = 2, 5000, 3
    X, y, k_lim, _, _, d, P = _site_problem('m4b_sg', D, 7, 11, K=1)
    eng = HipEngine('m4b_sg', X, y, k_lim)
    theta = ar1(np.random.RandomState(8), 1, chains, nkeep, P)
    got = eng.draw_diagnostics(theta=theta, chains=chains)
    exp = diagnostics_host(theta[0], chains)
    _close(got[0], exp, 1e-8, 'h = 2500')
    slow = np.arange(P) % 5 == 4                                        # phi = 0.99: ESS / n about 0.005
    assert np.all(got[0, slow, DG_ESS] < 0.03 * 10000) and np.all(got[0, ~slow, DG_ESS] > 0.03 * 10000)
    assert got.tobytes() == eng.draw_diagnostics(theta=theta, chains=chains).tobytes()
    eng.close()


# ------------------------------------------------------------------ (c) sites with several groups
@pytest.mark.parametrize('model,D,groups', [('m4b', 3, [[9], [8, 7, 9], [10, 6]]), ('m1b', 3, [[9], [8, 7, 9], [10, 6]]),
                                            ('m4b', 21, [[5], [4, 3, 4, 5, 3, 4]])])
def test_multi_group_sites_nan_behind_their_own_coordinates(model, D, groups):
    chains, nkeep, K = 4, 24, len(groups)
    X, y, k_lim, g_cnt, g_lim, _, _, d = _group_problem(model, D, groups, 23)
    eng = HipEngine(model, X, y, k_lim, g_cnt=g_cnt, g_lim=g_lim)
    assert len(set(eng.site_P)) > 1
    draws = ar1(np.random.RandomState(3), K, chains, nkeep, eng.P)
    theta = np.full_like(draws, np.nan)                                 # NaN behind every site's own coordinates
    for k in range(K):
        theta[k, :, :eng.site_P[k]] = draws[k, :, :eng.site_P[k]]
    got = eng.draw_diagnostics(theta=theta, chains=chains)
    for k in range(K):
        Pk = int(eng.site_P[k])
        assert np.all(np.isnan(got[k, Pk:])) and np.all(np.isfinite(got[k, :Pk]))
        _close(got[k, :Pk], diagnostics_host(theta[k, :, :Pk], chains), RTOL, 'site %d' % k)
    # what lies behind a site's coordinates plays no part
    assert np.array_equal(got, eng.draw_diagnostics(theta=np.where(np.isnan(theta), 1e300, theta), chains=chains),
                          equal_nan=True)
    eng.close()


# ------------------------------------------------------------------ (d) edge cases: results, never faults
def test_constant_nan_and_short_chains_give_nan_not_faults():
    K, chains, nkeep, D = 2, 4, 20, 3
    X, y, k_lim, _, _, d, P = _site_problem('m4b_sg', D, 7, 5, K=K)
    eng = HipEngine('m4b_sg', X, y, k_lim)
    theta = ar1(np.random.RandomState(4), K, chains, nkeep, P)
    ref = eng.draw_diagnostics(theta=theta, chains=chains)
    bad = theta.copy()
    bad[0, :, 1] = 2.5                                                  # a coordinate that never moved
    bad[1, :, 2] = np.repeat(np.arange(8.0), 10)                        # constant within every half chain
    bad[0, 7, 3] = np.nan
    bad[1, 50, 4] = np.inf
    got = eng.draw_diagnostics(theta=bad, chains=chains)
    hit = np.zeros((K, P), dtype=bool)
    hit[0, [1, 3]] = hit[1, [2, 4]] = True
    assert np.all(np.isnan(got[hit][:, NAN4]))
    assert got[~hit].tobytes() == ref[~hit].tobytes()                   # the other coordinates: untouched
    assert got[0, 1, DG_MEAN] == 2.5 and got[0, 1, DG_VAR] == 0.0
    assert got[1, 2, DG_MEAN] == 3.5 and got[1, 2, DG_VAR] == 6.0
    for k in range(K):
        _close(got[k], diagnostics_host(bad[k], chains), RTOL, 'site %d' % k)
    for short in (3, 2, 1):                                             # fewer than 4 draws per chain
        th = theta[:, :chains * short]
        got = eng.draw_diagnostics(theta=th, chains=chains)
        assert np.all(np.isnan(got[:, :, NAN4])) and np.all(np.isnan(got[:, :, DG_VAR]))
        for k in range(K):
            _close(got[k], diagnostics_host(th[k], chains), RTOL, 'nkeep = %d, site %d' % (short, k))
    eng.close()


# ------------------------------------------------------------------ (e) a coordinate far from zero: two-pass centring
@pytest.mark.parametrize('chains,nkeep', [(4, 100), (3, 401)])
def test_an_offset_coordinate_needs_the_centred_sums(chains, nkeep):
    """x = 1e6 + 1e-2 AR(1): centring in a second pass leaves about 2^-53 1e6 / 1e-2 = 1e-8 of the variance; a single
    pass (E x^2 - mean^2) would lose all of it."""
    K, D = 2, 3
    X, y, k_lim, _, _, d, P = _site_problem('m4b_sg', D, 7, 17, K=K)
    eng = HipEngine('m4b_sg', X, y, k_lim)
    theta = ar1(np.random.RandomState(nkeep), K, chains, nkeep, P)
    theta[:, :, 2] = 1e6 + 1e-2 * theta[:, :, 2]
    theta[:, :, 8] = 1e6 + 1e-2 * theta[:, :, 8]
    got = eng.draw_diagnostics(theta=theta, chains=chains)
    for k in range(K):
        exp = diagnostics_host(theta[k], chains)
        _close(got[k, [2, 8]], exp[[2, 8]], 1e-5, 'offset, site %d' % k)
        rest = np.setdiff1d(np.arange(P), [2, 8])
        _close(got[k, rest], exp[rest], RTOL, 'others, site %d' % k)
    eng.close()


# ------------------------------------------------------------------ (f) the sampler's own draws
def test_sampler_draws_on_the_device():
    D, K = 4, 6
    X, y, k_lim, Oms, mus, d, P = _site_problem('m4b_sg', D, 40, 41, K=K, tight=4.0)
    eng, _, _ = _engine_with_cavity('m4b_sg', X, y, k_lim, Oms, mus)
    with pytest.raises(_lib.EpxError, match='no draws yet'):            # nothing sampled yet
        eng.draw_diagnostics()
    opts = HipEngine.sampler_opts(chains=4, iter=24, warmup=None, init='random')
    stats, _ = eng.sample_batch(np.arange(11, 11 + K, dtype=np.int64), opts)
    got, n = eng.draw_diagnostics(with_n=True)
    assert got.shape == (K, P, DG_COUNT) and n == 48 and np.all(np.isfinite(got))
    assert got.tobytes() == eng.draw_diagnostics().tobytes()            # twice: the same bits
    draws = np.stack([np.ascontiguousarray(eng.get_draws(k, all_params=True)) for k in range(K)])
    assert draws.shape == (K, 48, P)
    assert got.tobytes() == eng.draw_diagnostics(theta=draws, chains=4).tobytes()
    for k in range(K):
        _close(got[k], diagnostics_host(draws[k], 4), RTOL, 'site %d' % k)
    # the one number per site the sampling call reports is the largest of these
    np.testing.assert_allclose(got[:, :, DG_RHAT].max(axis=1), stats[:, 1], rtol=1e-12)
    assert eng.draw_diagnostics(k0=2, count=3).tobytes() == got[2:5].tobytes()
    eng.sample_batch(np.array([5, 6], dtype=np.int64), opts, k0=1, count=2)     # only sites 1, 2 are current now
    assert eng.draw_diagnostics(k0=1, count=2).shape == (2, P, DG_COUNT)
    with pytest.raises(_lib.EpxError, match='left draws of sites'):
        eng.draw_diagnostics()
    eng.close()


# ------------------------------------------------------------------ (g) errors, not faults
def test_bad_arguments_are_errors():
    K, D = 3, 3
    X, y, k_lim, _, _, d, P = _site_problem('m4b_sg', D, 7, 5, K=K)
    eng = HipEngine('m4b_sg', X, y, k_lim)
    theta = np.random.RandomState(0).randn(K, 40, P)
    assert eng.draw_diagnostics(theta=theta, chains=4).shape == (K, P, DG_COUNT)
    with pytest.raises(_lib.EpxError, match='no multiple of chains'):
        eng.draw_diagnostics(theta=theta, chains=3)
    for chains in (0, -1, 17):
        with pytest.raises(_lib.EpxError, match='chains must be in'):
            eng.draw_diagnostics(theta=theta, chains=chains)
    with pytest.raises(ValueError, match='chains'):
        eng.draw_diagnostics(theta=theta)
    with pytest.raises(ValueError, match='theta'):
        eng.draw_diagnostics(theta=theta[:, :, :-1], chains=4)
    for k0, count in ((-1, 2), (2, 2), (0, 0), (3, 1)):
        with pytest.raises(_lib.EpxError, match='site range'):
            eng.draw_diagnostics(k0=k0, count=count, theta=theta[:max(count, 0)], chains=4)
    eng.close()


# ------------------------------------------------------------------ (h) Master.diagnostics on the device
@pytest.mark.parametrize('J,K', [(4, 4), (5, 3)])
def test_master_diagnostics_on_the_device(J, K):
    D = 3
    conf = fit.configurations(J=J, D=D, K=K, npg=30, siter=40, run_ep=True, damp=0.4)
    M = fit.main('m4b', conf, ret_master=True)
    assert isinstance(M.engine, HipEngine)
    with pytest.raises(RuntimeError, match='at least one iteration'):
        M.diagnostics()
    assert M.run(2, verbose=False, calc_moments=False, seed=5) == 0
    multi = not M.model_name.endswith('_sg')
    assert multi == (K < J)
    res = M.diagnostics()
    chains = M.workers[0].stan_params['chains']
    S = M.engine.num_draws()
    assert np.all(res['n'] == 2 * chains * (S // chains // 2)) and res['mean'].shape == (K, M.engine.P)
    names = ('mean', 'var', 'rhat', 'ess', 'mcse', 'ess_sq')
    for k in range(K):
        Pk = int(M.engine.site_P[k]) if multi else M.engine.P
        exp = diagnostics_host(np.ascontiguousarray(M.engine.get_draws(k, all_params=True))[:, :Pk], chains)
        got = np.stack([res[name][k] for name in names], axis=1)
        assert np.all(np.isnan(got[Pk:])) and np.all(np.isfinite(got[:Pk]))
        _close(got[:Pk], exp, RTOL, 'site %d' % k)
    np.testing.assert_array_equal(res['site_max_rhat'], np.nanmax(res['rhat'], axis=1))
    emin = np.nanmin(np.minimum(res['ess'], res['ess_sq']), axis=1)
    np.testing.assert_array_equal(res['site_min_ess'], emin)
    k, e = res['worst']
    assert k == int(np.argmin(emin)) and min(res['ess'][k, e], res['ess_sq'][k, e]) == emin.min()
    # the sampler's one number per site is the largest of these
    np.testing.assert_allclose(res['site_max_rhat'], M.last_site_stats[:, 1], rtol=1e-12)


# ------------------------------------------------------------------ (i) a stand-alone Worker
def test_stand_alone_worker_diagnostics():
    rng = np.random.RandomState(13)
    X, y, d = rng.randn(20, 4), (rng.rand(20) < 0.5).astype(int), 10
    w = Worker(0, 'none/m4b_sg', d, X, y, chains=4, iter=40)
    A = rng.randn(d, d + 3)
    Q = np.asfortranarray(A.dot(A.T) / (d + 3) + 2.0 * np.eye(d))
    assert w.cavity(Q, rng.randn(d), np.zeros((d, d), order='F'), np.zeros(d))
    with pytest.raises(RuntimeError, match='before `tilted`'):
        w.diagnostics()
    w.tilted(np.zeros((d, d), order='F'), np.zeros(d), seed=7)
    rec = w.diagnostics()
    P = w._eng.P
    assert rec.shape == (P, DG_COUNT) and np.all(np.isfinite(rec))
    _close(rec, diagnostics_host(np.ascontiguousarray(w._eng.get_draws(0, all_params=True)), 4), RTOL, 'worker')
    np.testing.assert_allclose(rec[:, DG_RHAT].max(), w.last_mrhat, rtol=1e-12)
