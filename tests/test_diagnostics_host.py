"""`diagnostics.diagnostics_host` and `Master.diagnostics` on the CPU: the NumPy statement of the per-coordinate
diagnostics (include/epx.h, enum epx_diag) against a brute-force loop written straight from the definition, its edge
cases, its statistical meaning on AR(1) chains whose effective sample size is known, and `Master.diagnostics`'
bookkeeping with the oracle standing in for the device engine, on one rank and on two over gloo."""

import math
import os
import sys

import numpy as np
import pytest

from epstan_amd import diagnostics as dg
from epstan_amd.diagnostics import DG_ESS, DG_ESS_SQ, DG_MCSE, DG_MEAN, DG_RHAT, DG_VAR, diagnostics_host

import test_predict_host as tph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN4 = [DG_RHAT, DG_ESS, DG_MCSE, DG_ESS_SQ]


def ar1(rng, phi, chains, nkeep, P=None):
    """(chains * nkeep, P) chain-major stationary AR(1) draws with unit innovation variance; phi a scalar or (P)."""
    phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), (P if P is not None else np.size(phi),))
    x = np.empty((chains, nkeep, phi.shape[0]))
    x[:, 0] = rng.randn(chains, phi.shape[0]) / np.sqrt(1 - phi ** 2)
    for t in range(1, nkeep):
        x[:, t] = phi * x[:, t - 1] + rng.randn(chains, phi.shape[0])
    return x.reshape(chains * nkeep, -1)


# ------------------------------------------------------------------ the definition, in loops
def _brute_ess(halves):
    """(MEAN, var_plus, W, ESS) of ONE coordinate's half chains (lists of floats), math.fsum everywhere."""
    M, h = len(halves), len(halves[0])
    n = M * h
    means = [math.fsum(c) / h for c in halves]
    dev = [[v - means[m] for v in c] for m, c in enumerate(halves)]

    def acov(t):
        return math.fsum(math.fsum(d[i] * d[i + t] for i in range(h - t)) / h for d in dev) / M

    W = math.fsum(math.fsum(v * v for v in d) / h * h / (h - 1) for d in dev) / M
    mean = math.fsum(means) / M
    var_plus = W * (h - 1) / h + math.fsum((m - mean) ** 2 for m in means) / (M - 1)
    if not (math.isfinite(W) and W > 0):
        return mean, var_plus, W, float('nan')

    def rho(t):
        return 1 - (W - acov(t)) / var_plus

    pairs, j = [], 0
    while 2 * j + 1 < h:
        p = (1.0 if j == 0 else rho(2 * j)) + rho(2 * j + 1)
        if not p > 0:
            break
        pairs.append(min(p, pairs[-1]) if pairs else p)
        j += 1
    tau = max(-1 + 2 * math.fsum(pairs), 1 / math.log10(n))
    return mean, var_plus, W, n / tau


def _brute(theta, chains):
    S, P = theta.shape
    nkeep = S // chains
    h = nkeep // 2
    out = np.full((P, 6), np.nan)
    for e in range(P):
        x = theta[:, e].reshape(chains, nkeep)
        halves = [list(map(float, part)) for c in range(chains) for part in (x[c, :h], x[c, nkeep - h:])]
        mean, var_plus, W, ess = _brute_ess(halves)
        _, _, _, ess_sq = _brute_ess([[(v - mean) ** 2 for v in c] for c in halves])
        out[e] = [mean, var_plus, math.sqrt(var_plus / W), ess, math.sqrt(var_plus / ess), ess_sq]
    return out


@pytest.mark.parametrize('chains,nkeep', [(1, 4), (2, 5), (4, 9), (4, 100), (3, 401)])
def test_diagnostics_host_against_the_definition_in_loops(chains, nkeep):
    rng = np.random.RandomState(100 * chains + nkeep)
    phi = np.array([-0.5, 0.0, 0.5, 0.9, 0.99])
    theta = ar1(rng, phi, chains, nkeep) + np.array([0.0, 3.0, -1.0, 10.0, 0.5])
    got = diagnostics_host(theta, chains)
    assert got.shape == (5, 6) and dg.DG_COUNT == 6
    np.testing.assert_allclose(got, _brute(theta, chains), rtol=1e-12)
    assert np.all(np.isfinite(got)) and np.all(got[:, DG_ESS] > 0) and np.all(got[:, DG_ESS_SQ] > 0)


# ------------------------------------------------------------------ edge cases
def test_fewer_than_four_draws_per_chain_give_nan():
    rng = np.random.RandomState(0)
    for nkeep in (1, 2, 3):
        theta = rng.randn(4 * nkeep, 3)
        got = diagnostics_host(theta, 4)
        assert np.all(np.isnan(got[:, NAN4])) and np.all(np.isnan(got[:, DG_VAR]))
    x = theta.reshape(4, 3, 3)                           # nkeep = 3: the middle draw is dropped
    np.testing.assert_allclose(got[:, DG_MEAN], x[:, [0, 2]].mean(axis=(0, 1)), rtol=1e-14)


def test_constant_and_non_finite_coordinates_give_nan_for_themselves_only():
    rng = np.random.RandomState(1)
    theta = rng.randn(4 * 20, 5)
    ref = diagnostics_host(theta, 4)
    bad = theta.copy()
    bad[:, 1] = 2.5                                      # a chain that never moved, everywhere
    bad[7, 2] = np.nan
    bad[50, 3] = np.inf
    got = diagnostics_host(bad, 4)
    for e in (1, 2, 3):
        assert np.all(np.isnan(got[e, NAN4])), e
    assert got[1, DG_MEAN] == 2.5 and got[1, DG_VAR] == 0.0
    np.testing.assert_array_equal(got[[0, 4]], ref[[0, 4]])
    # constant within every half chain, at different levels: W = 0 all the same
    bad[:, 1] = np.repeat(np.arange(8.0), 10)
    got = diagnostics_host(bad, 4)
    assert np.all(np.isnan(got[1, NAN4])) and got[1, DG_MEAN] == 3.5 and got[1, DG_VAR] == 6.0


def test_one_chain_is_well_defined():
    theta = ar1(np.random.RandomState(2), 0.3, 1, 200, P=2)
    got = diagnostics_host(theta, 1)
    assert np.all(np.isfinite(got)) and np.all(got[:, DG_RHAT] < 1.1)
    with pytest.raises(ValueError, match='multiple of chains'):
        diagnostics_host(theta[:-1], 3)


# ------------------------------------------------------------------ what the numbers mean
@pytest.mark.parametrize('phi,lo,hi', [(0.0, 0.95, 1.05), (0.5, 0.303, 0.363), (0.9, 0.043, 0.063), (-0.5, 2.0, np.inf)])
def test_ess_of_ar1_chains(phi, lo, hi):
    """ESS / n of an AR(1) chain is (1 - phi) / (1 + phi); antithetic chains are not capped at n."""
    theta = ar1(np.random.RandomState(20261019), phi, 4, 2000, P=16)
    got = diagnostics_host(theta, 4)
    ratio = float(np.mean(got[:, DG_ESS] / 8000))
    print('phi = %g: mean ESS / n = %.4f (theory %.4f)' % (phi, ratio, (1 - phi) / (1 + phi)))
    assert lo < ratio < hi
    np.testing.assert_allclose(got[:, DG_MCSE], np.sqrt(got[:, DG_VAR] / got[:, DG_ESS]), rtol=1e-14)


def test_rhat_of_mixed_and_of_offset_chains():
    rng = np.random.RandomState(5)
    theta = rng.randn(4, 200, 6)
    mixed = diagnostics_host(theta.reshape(800, 6), 4)
    assert np.all(mixed[:, DG_RHAT] < 1.05)
    theta[1] += 3.0                                      # one chain 3 sd away
    apart = diagnostics_host(theta.reshape(800, 6), 4)
    assert np.all(apart[:, DG_RHAT] > 1.5)
    assert np.all(apart[:, DG_ESS] < 0.1 * mixed[:, DG_ESS])


# ------------------------------------------------------------------ Master.diagnostics
def test_summary_skips_nan_and_keeps_an_all_nan_site_nan():
    rec = np.full((3, 4, 6), np.nan)
    rec[0, :2] = [[0.0, 1.0, 1.01, 50.0, 0.1, 70.0], [0.0, 1.0, 1.20, 90.0, 0.1, 30.0]]
    rec[2, :3, :] = [0.0, 1.0, 1.05, 40.0, 0.1, 45.0]
    rec[2, 1, NAN4] = np.nan                             # a constant coordinate among good ones
    res = dg.summarise(rec, [80, 80, 80])
    np.testing.assert_array_equal(res['site_max_rhat'], [1.20, np.nan, 1.05])
    np.testing.assert_array_equal(res['site_min_ess'], [30.0, np.nan, 40.0])
    assert res['worst'] == (0, 1)
    assert dg.summarise(np.full((2, 3, 6), np.nan), [4, 4])['worst'] is None


def _expected_records(M, chains=4):
    """diagnostics_host on the engine's downloaded draws, site by site, NaN behind a site's own coordinates."""
    eng = M.engine
    pg = (eng.P - eng.d) // int(M._site_ng[M.k_lo:M.k_hi].max())
    site_P = eng.d + M._site_ng * pg
    rec = np.full((M.K, int(site_P.max()), 6), np.nan)
    for k in range(M.K):
        theta = np.ascontiguousarray(eng.get_draws(k, all_params=True))[:, :site_P[k]]
        rec[k, :site_P[k]] = diagnostics_host(theta, chains)
    return rec, site_P


def _check_summary(res, rec, K):
    for i, name in enumerate(('mean', 'var', 'rhat', 'ess', 'mcse', 'ess_sq')):
        np.testing.assert_array_equal(res[name], rec[:, :, i])
    np.testing.assert_array_equal(res['site_max_rhat'], np.nanmax(rec[:, :, DG_RHAT], axis=1))
    emin = np.nanmin(np.minimum(rec[:, :, DG_ESS], rec[:, :, DG_ESS_SQ]), axis=1)
    np.testing.assert_array_equal(res['site_min_ess'], emin)
    k, e = res['worst']
    assert k == int(np.argmin(emin)) and min(rec[k, e, DG_ESS], rec[k, e, DG_ESS_SQ]) == emin.min()
    assert res['n'].shape == (K,) and res['n'].dtype == np.int64


def test_master_diagnostics_single_group():
    M, data = tph._sg_master()
    with pytest.raises(RuntimeError, match='at least one iteration'):
        M.diagnostics()
    info, (stimes, msteps, mrhats, othertimes) = M.run(1, verbose=False, calc_moments=False, return_analytics=True, seed=2)
    assert info == M.INFO_OK
    res = M.diagnostics()
    assert set(res) == {'mean', 'var', 'rhat', 'ess', 'ess_sq', 'mcse', 'n', 'site_max_rhat', 'site_min_ess', 'worst'}
    rec, site_P = _expected_records(M)
    assert rec.shape == (4, M.engine.P, 6) and np.all(np.isfinite(rec))
    _check_summary(res, rec, 4)
    assert np.all(res['n'] == 80)
    # the one number per site the sampler reports is the largest of these
    np.testing.assert_allclose(res['site_max_rhat'], M.last_site_stats[:, 1], rtol=1e-12)
    np.testing.assert_allclose(res['site_max_rhat'].max(), mrhats[-1], rtol=1e-12)
    # the tilted mean the update used is the mean of ALL draws; with an even nkeep the half chains hold them all
    np.testing.assert_allclose(res['mean'][2, :M.dphi], M.engine.get_draws(2).mean(axis=0), rtol=1e-12)

    def from_cavity(data, stan_params):                  # draws of phi alone, as an injector gives them
        z = np.random.RandomState(stan_params['seed'] % 1000).randn(80, 6)
        return data['mu_phi'] + np.linalg.solve(np.linalg.cholesky(data['Omega_phi']).T, z.T).T
    M._sample_injector = from_cavity
    M.run(1, verbose=False, seed=3)
    with pytest.raises(RuntimeError, match='injected'):
        M.diagnostics()


def test_master_diagnostics_with_several_groups_per_site():
    M, data, Nk, j_ind = tph._groups_master()            # 7 groups on 3 sites: 3 + 2 + 2
    M.run(1, verbose=False, seed=3)
    res = M.diagnostics()
    rec, site_P = _expected_records(M)
    assert len(set(site_P)) > 1 and rec.shape[1] == M.engine.P
    for k in range(3):                                   # NaN exactly behind the site's own coordinates
        assert np.all(np.isfinite(res['ess'][k, :site_P[k]])) and np.all(np.isnan(res['ess'][k, site_P[k]:]))
        assert np.all(np.isfinite(res['mean'][k, :site_P[k]])) and np.all(np.isnan(res['mean'][k, site_P[k]:]))
    _check_summary(res, rec, 3)


# ------------------------------------------------------------------ two ranks over gloo
KEYS = ('mean', 'var', 'rhat', 'ess', 'ess_sq', 'mcse', 'n', 'site_max_rhat', 'site_min_ess', 'worst')


def _worker(rank, world, port, outdir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['RANK'] = str(rank)
    os.environ['WORLD_SIZE'] = str(world)
    for p in (ROOT, os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as tdist
    from epstan_amd import dist
    from oracle.engine_oracle import OracleEngine
    import test_predict_host as me
    tdist.init_process_group('gloo', rank=rank, world_size=world)
    fac = lambda m, X, y, kl, **g: OracleEngine(m, X, y, kl, nthreads=2, **g)
    M, data, Nk, j_ind = me._groups_master(comm=dist.TorchComm(), _engine_factory=fac)
    M.run(1, verbose=False, seed=3)
    res = M.diagnostics()
    np.savez(os.path.join(outdir, 'r%d.npz' % rank), **dict((k, np.asarray(res[k])) for k in KEYS))
    tdist.barrier()
    tdist.destroy_process_group()


def test_two_ranks_diagnostics_equal_one_rank(tmp_path):
    """7 groups on 3 sites, sharded 1 + 2 (the ranks' record strides differ): every rank computes its own sites, the
    records are gathered, NaN padding included, and both ranks return what one rank returns, bit for bit."""
    import torch.multiprocessing as mp
    from oracle.engine_oracle import OracleEngine
    mp.spawn(_worker, args=(2, tph._free_port(), str(tmp_path)), nprocs=2, join=True)
    M, data, Nk, j_ind = tph._groups_master(
        _engine_factory=lambda m, X, y, kl, **g: OracleEngine(m, X, y, kl, nthreads=2, **g))
    M.run(1, verbose=False, seed=3)
    res = M.diagnostics()
    assert np.isnan(res['ess']).any() and np.all(np.isfinite(res['site_min_ess']))
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), 'r%d.npz' % r))
        for key in KEYS:
            np.testing.assert_array_equal(z[key], np.asarray(res[key]), err_msg=key)
