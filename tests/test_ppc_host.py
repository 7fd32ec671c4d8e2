"""ppc.py, the NumPy statement of the posterior predictive checks (include/epx.h, enum epx_ppc), and `Master.ppc` on the
CPU: the statement against a plain loop over (group, row, draw) that draws every cell's replicate on its own, its
calibration on data simulated from the model, the exact tie of the two discrepancies, the summary, the two routes'
signatures, and `Master.ppc` with the oracle standing in for the device engine, on one rank and on two over gloo."""

import inspect
import math
import os
import sys

import numpy as np
import pytest

import test_predict_host as tph
from epstan_amd import draw_queries as dq, newgroup, ppc, site_params
from epstan_amd.engine import HipEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = ppc.PC_COUNT


def _n_params(mid, D, ng, gauss):
    return site_params.layout(mid, D, ng, gauss)[1] + ng * (1 + (D if mid else 0))


# ------------------------------------------------------------------ the statement against a loop over cells
def _cell_uniforms(seed, s, a):
    o = newgroup.philox4x32(newgroup.make_key(seed, 0), s, ppc.K_PPC, a, 0)
    return float(newgroup.u01(o[0], o[1])), float(newgroup.u01(o[2], o[3]))


def _loop(mid, D, site_ng, gauss, thetas, X, group, y, k_lim, seed, row0):
    """(groups, sites, draws) by a triple loop: one Philox call per (group, row, draw), sums added one by one."""
    groups, sites, draws = [], [], []
    for k, ng in enumerate(site_ng):
        lo, hi = int(k_lim[k]), int(k_lim[k + 1])
        theta = thetas[k]
        S = theta.shape[0]
        grp = np.zeros(hi - lo, dtype=int) if group is None else group[lo:hi]
        f = site_params.linear_predictor(mid, D, ng, gauss, theta, X[lo:hi], grp)
        per = np.zeros((ng, 3, S))
        t_obs = np.zeros(ng)
        for g in range(ng):
            for i in np.nonzero(grp == g)[0]:
                row = row0 + lo + int(i)
                t_obs[g] += y[lo + i]
                for s in range(S):
                    fis = float(f[s, i])
                    if gauss:
                        sigma = math.exp(theta[s, 0])
                        u1, u2 = _cell_uniforms(seed, s, row >> 1)
                        rad, ang = math.sqrt(-2.0 * math.log(u1)), 6.283185307179586476925286766559 * u2
                        y_rep = fis + sigma * (rad * math.sin(ang) if row & 1 else rad * math.cos(ang))

                        def ll(v):
                            return -0.5 * math.log(2 * math.pi) - theta[s, 0] - 0.5 * ((v - fis) / sigma) ** 2
                    else:
                        u1, _ = _cell_uniforms(seed, s, row)
                        y_rep = 1.0 if u1 < 1.0 / (1.0 + math.exp(-fis)) else 0.0

                        def ll(v):
                            return v * fis - (max(fis, 0.0) + math.log1p(math.exp(-abs(fis))))
                    per[g, 0, s] += y_rep
                    per[g, 1, s] += ll(float(y[lo + i]))
                    per[g, 2, s] += ll(y_rep)

        def rec(unit, t):
            mean = unit[0].sum() / S
            return [t, mean, ((unit[0] - mean) ** 2).sum(), (unit[0] >= t).sum(), (unit[0] > t).sum(), unit[1].sum() / S,
                    unit[2].sum() / S, (unit[2] <= unit[1]).sum()]
        groups += [rec(per[g], t_obs[g]) for g in range(ng)]
        sites.append(rec(per.sum(axis=0), t_obs.sum()))
        draws.append(per)
    return np.array(groups, dtype=float), np.array(sites, dtype=float), np.concatenate(draws)


def _problem(mid, gauss, sizes, D, S, seed):
    """Sites with the group sizes `sizes` (a list per site), random rows, responses and draws."""
    rng = np.random.RandomState(seed)
    site_ng = [len(s) for s in sizes]
    k_lim = np.concatenate(([0], np.cumsum([sum(s) for s in sizes])))
    N = int(k_lim[-1])
    X = 1.2 * rng.randn(N, D)
    y = 0.3 + rng.randn(N) if gauss else (rng.rand(N) < 0.5).astype(float)
    group = np.concatenate([np.repeat(np.arange(len(s)), s) for s in sizes])
    thetas = [0.5 * rng.randn(S, _n_params(mid, D, ng, gauss)) + 0.2 for ng in site_ng]
    return site_ng, k_lim, X, y, group, thetas


@pytest.mark.parametrize('mid,gauss,sizes', [(0, False, [[5], [4]]), (3, False, [[3, 1], [2, 4, 2]]), (3, True, [[2, 3], [4]])],
                         ids=['m1b_sg', 'm4b', 'm4a'])
def test_ppc_host_against_a_loop_over_cells(mid, gauss, sizes):
    D, S, seed, row0 = 2, 7, 12345678901234567, 5
    site_ng, k_lim, X, y, group, thetas = _problem(mid, gauss, sizes, D, S, 40 + mid + gauss)
    single = all(ng == 1 for ng in site_ng)
    got = ppc.ppc_host(mid, D, site_ng, gauss, thetas, X, None if single else group, y, k_lim, seed, row0)
    exp = _loop(mid, D, site_ng, gauss, thetas, X, None if single else group, y, k_lim, seed, row0)
    G = sum(site_ng)
    assert got[0].shape == (G, C) and got[1].shape == (len(sizes), C) and got[2].shape == (G, 3, S)
    for g, e, what in zip(got, exp, ('groups', 'sites', 'draws')):
        np.testing.assert_allclose(g, e, rtol=1e-12, atol=1e-13, err_msg=what)
    counts = [ppc.PC_T_GE, ppc.PC_T_GT, ppc.PC_D_LE]
    np.testing.assert_array_equal(got[0][:, counts], exp[0][:, counts])
    if not gauss:                                          # integers: exact
        np.testing.assert_array_equal(got[2][:, 0], exp[2][:, 0])
        np.testing.assert_array_equal(got[0][:, :2], exp[0][:, :2])
    if single:                                             # the site repeats its one group
        np.testing.assert_array_equal(got[0], got[1])
    # a replicate is a function of (seed, row, draw): a site alone, with its rows' place in the stream, gives its bits
    lo, hi = int(k_lim[1]), int(k_lim[2])
    alone = ppc.ppc_host(mid, D, site_ng[1:], gauss, thetas[1:], X[lo:hi], None if single else group[lo:hi], y[lo:hi],
                         k_lim[1:] - lo, seed, row0 + lo)
    np.testing.assert_array_equal(alone[0], got[0][site_ng[0]:])
    np.testing.assert_array_equal(alone[1], got[1][1:])
    other = ppc.ppc_host(mid, D, site_ng, gauss, thetas, X, None if single else group, y, k_lim, seed + 1, row0)
    assert np.any(other[2][:, 0] != got[2][:, 0])


def test_a_non_finite_cell_makes_its_group_and_site_nan():
    site_ng, k_lim, X, y, group, thetas = _problem(3, False, [[3, 2], [4]], 2, 9, 3)
    good = ppc.ppc_host(3, 2, site_ng, False, thetas, X, group, y, k_lim)
    d = site_params.layout(3, 2, 2, False)[1]
    thetas[0][4, d + 1] = np.nan                          # eta of group 1 of site 0 in one draw
    got = ppc.ppc_host(3, 2, site_ng, False, thetas, X, group, y, k_lim)
    assert np.all(np.isnan(got[0][1])) and np.all(np.isnan(got[1][0]))
    np.testing.assert_array_equal(got[0][[0, 2]], good[0][[0, 2]])
    np.testing.assert_array_equal(got[1][1], good[1][1])


# ------------------------------------------------------------------ calibration
@pytest.mark.parametrize('gauss', [False, True], ids=['bernoulli', 'gaussian'])
def test_p_values_are_uniform_on_data_simulated_from_the_model(gauss):
    """Every draw of a site IS the simulating parameter and y comes from the same model (NumPy's generator, not the
    stream): p_t and p_d are uniform, the mean of G of them lies within 4 standard deviations of a uniform mean."""
    G, n, D, S, mid = 400, 30, 2, 64, 3
    rng = np.random.RandomState(2024)
    P = _n_params(mid, D, 1, gauss)
    X = rng.randn(G * n, D)
    k_lim = np.arange(G + 1) * n
    truth = 0.5 * rng.randn(G, P)
    thetas = [np.repeat(truth[k][None, :], S, axis=0) for k in range(G)]
    y = np.empty(G * n)
    for k in range(G):
        f = site_params.linear_predictor(mid, D, 1, gauss, truth[k][None, :], X[k * n:(k + 1) * n], None)[0]
        y[k * n:(k + 1) * n] = f + math.exp(truth[k, 0]) * rng.randn(n) if gauss else rng.rand(n) < ppc.sigmoid(f)
    groups, sites, _ = ppc.ppc_host(mid, D, [1] * G, gauss, thetas, X, None, y, k_lim, seed=7)
    res = ppc.summarise(groups, sites, S, [1] * G)
    bound = 4.0 / math.sqrt(12 * G)
    print('mean p_t %.4f, mean p_d %.4f, bound 0.5 +- %.4f' % (res['p_t'].mean(), res['p_d'].mean(), bound))
    assert abs(res['p_t'].mean() - 0.5) <= bound
    assert abs(res['p_d'].mean() - 0.5) <= bound


def test_a_group_of_ones_at_even_odds_is_extreme():
    n, D, S = 30, 2, 200
    theta = np.zeros((S, _n_params(0, D, 1, False)))      # m1b_sg at 0: f = 0, sigmoid(f) = 1 / 2
    X = np.random.RandomState(0).randn(n, D)
    groups, sites, _ = ppc.ppc_host(0, D, [1], False, [theta], X, None, np.ones(n), np.array([0, n]))
    res = ppc.summarise(groups, sites, S, [1])
    assert res['t_obs'][0] == n and abs(res['t_rep_mean'][0] - n / 2) < 1.0
    assert res['p_t_ge'][0] < 2.0 / S and res['extreme'].tolist() == [0]


# ------------------------------------------------------------------ the exact tie
def test_draws_that_replicate_the_data_tie_the_two_discrepancies_to_the_bit():
    D, S = 3, 64
    rng = np.random.RandomState(8)
    theta = 0.5 * rng.randn(S, _n_params(3, D, 1, False))
    X, y, rows = rng.randn(2, D), np.array([1.0, 0.0]), np.array([10, 11])
    f, y_rep, ll_obs, ll_rep = ppc.site_cells(3, D, 1, False, theta, X, None, y, 4, rows)
    per, t_obs, bad = ppc.site_per_draw(3, D, 1, False, theta, X, None, y, 4, rows)
    tie = np.all(y_rep == y[None, :], axis=1)
    assert 4 <= tie.sum() <= S - 4
    assert np.all(per[0, ppc.PD_D_REP][tie] == per[0, ppc.PD_D_OBS][tie])
    assert np.all(per[0, ppc.PD_D_REP][~tie] != per[0, ppc.PD_D_OBS][~tie])
    rec = ppc.record(per[0], t_obs[0], bad[0])
    below = int(np.count_nonzero(per[0, ppc.PD_D_REP][~tie] < per[0, ppc.PD_D_OBS][~tie]))
    assert rec[ppc.PC_D_LE] == below + tie.sum()          # the ties count


# ------------------------------------------------------------------ the summary
def test_summary_turns_counts_into_p_values():
    S, site_ng = 40, [2, 1]
    groups = np.array([[3.0, 2.5, 39.0, 20, 10, -7.0, -7.5, 4],
                       [1.0, 1.0, 0.0, 40, 38, -2.0, -2.1, 39],
                       [np.nan] * 8])
    sites = np.array([[4.0, 3.5, 78.0, 30, 20, -9.0, -9.6, 20], [np.nan] * 8])
    res = ppc.summarise(groups, sites, S, site_ng, level=0.1)
    assert res['n'] == S and res['level'] == 0.1 and res['group_site'].tolist() == [0, 0, 1]
    np.testing.assert_array_equal(res['p_t_ge'][:2], [0.5, 1.0])
    np.testing.assert_array_equal(res['p_t'][:2], [30 / 80.0, 78 / 80.0])
    np.testing.assert_array_equal(res['p_d'][:2], [0.1, 39 / 40.0])
    np.testing.assert_array_equal(res['t_rep_var'][:2], [1.0, 0.0])
    np.testing.assert_array_equal(res['site_p_t'][:1], [50 / 80.0])
    np.testing.assert_array_equal(res['site_t_rep_var'][:1], [2.0])
    assert res['t_obs'][0] == 3.0 and res['d_obs_mean'][1] == -2.0 and res['d_rep_mean'][1] == -2.1
    for key in ('p_t', 'p_d', 'p_t_ge', 't_obs'):
        assert np.isnan(res[key][2]) and np.isnan(res['site_' + key][1])
    assert res['extreme'].tolist() == [1]                  # p_t = 0.975 > 0.95; the NaN group is not listed
    assert ppc.summarise(groups, sites, S, site_ng, level=0.3)['extreme'].tolist() == [0, 1]     # p_d = 0.1 < 0.15
    assert 'draws' not in res and ppc.summarise(groups, sites, S, site_ng, draws=np.zeros((3, 3, S)))['draws'].shape == (3, 3, S)
    with pytest.raises(ValueError, match='level'):
        ppc.summarise(groups, sites, S, site_ng, level=1.0)


# ------------------------------------------------------------------ the two routes, Master.ppc
class Recorder(object):
    """Stands in for `Master._queries`: notes (name, args, kwargs) of every call and passes it on."""

    def __init__(self, target):
        self.target, self.calls = target, []

    def __getattr__(self, name):
        def call(*args, **kw):
            self.calls.append((name, args, kw))
            return getattr(self.target, name)(*args, **kw)
        return call


@pytest.fixture(scope='module')
def fitted():
    M, data, Nk, j_ind = tph._groups_master()              # m4b, 7 groups on 3 sites: 3 + 2 + 2
    with pytest.raises(RuntimeError, match='before at least one iteration'):
        M.ppc()
    M.run(1, verbose=False, seed=3)
    return M


def test_checks_is_a_tuple_of_its_own():
    assert dq.CHECKS == ('replicated_checks',) and len(dq.QUERIES) == 8 and not set(dq.CHECKS) & set(dq.QUERIES)


@pytest.mark.parametrize('name', dq.CHECKS)
def test_the_host_route_keeps_the_engines_signature(name, fitted):
    M = fitted
    resolver = M._queries
    rec = M._queries = Recorder(resolver)
    try:
        M.ppc()
        M.ppc(seed=9, level=0.2, draws=True)
    finally:
        M._queries = resolver
    assert sorted(set(called for called, _, _ in rec.calls)) == sorted(dq.CHECKS)     # the engine is reached as this only
    host, device = inspect.signature(getattr(dq.HostDraws, name)), inspect.signature(getattr(HipEngine, name))
    for par in host.parameters.values():
        assert par.name in device.parameters, '%s: HipEngine.%s takes no `%s`' % (name, name, par.name)
        assert par.default == device.parameters[par.name].default, (name, par.name)
    assert len(rec.calls) == 2
    for _, args, kw in rec.calls:                          # every argument lands on the same name on both routes
        to_host, to_device = host.bind('self', *args, **kw).arguments, device.bind('self', *args, **kw).arguments
        assert list(to_host) == list(to_device) and all(to_host[k] is to_device[k] for k in to_host), name


def test_the_resolver_prefers_the_engines_own_method(fitted):
    M = fitted
    assert not hasattr(M.engine, 'replicated_checks')
    assert M._queries.replicated_checks.__func__ is dq.HostDraws.replicated_checks
    M.engine.replicated_checks = lambda **kw: 'the engine'
    try:
        assert M._queries.replicated_checks(seed=1) == 'the engine'
    finally:
        del M.engine.replicated_checks


KEYS = ('group_site', 't_obs', 't_rep_mean', 't_rep_var', 'p_t_ge', 'p_t', 'd_obs_mean', 'd_rep_mean', 'p_d')


def test_master_ppc_on_the_host_route(fitted):
    M = fitted
    res = M.ppc(seed=5, draws=True)
    G, K, S = 7, 3, M.engine.num_draws()
    assert set(res) == set(KEYS) | set('site_' + k for k in KEYS[1:]) | {'n', 'level', 'extreme', 'draws'}
    assert res['n'] == S and res['draws'].shape == (G, 3, S)
    assert sorted(M._site_ng) == [2, 2, 3] and res['group_site'].tolist() == np.repeat(np.arange(K), M._site_ng).tolist()
    for key in KEYS:
        assert res[key].shape == (G,), key
    for key in KEYS[1:]:
        assert res['site_' + key].shape == (K,) and np.all(np.isfinite(res['site_' + key])), key
    # the statement on the engine's draws, with the Master's rows and groups
    mid, gauss, _ = M._site_spec()
    thetas = [M.engine.get_draws(k, all_params=True) for k in range(K)]
    groups, sites, draws = ppc.ppc_host(mid, M.D, M._site_ng, gauss, thetas, M.X, np.asarray(M.A_n['j_ind']) - 1, M.y,
                                        M.k_lim, seed=5)
    np.testing.assert_array_equal(res['draws'], draws)
    np.testing.assert_array_equal(res['p_t'], (groups[:, ppc.PC_T_GE] + groups[:, ppc.PC_T_GT]) / (2.0 * S))
    np.testing.assert_array_equal(res['site_p_d'], sites[:, ppc.PC_D_LE] / S)
    # the observed sums are the data's; a site's per-draw values are its groups'
    first = np.concatenate(([0], np.cumsum(M._site_ng)))
    np.testing.assert_array_equal(res['site_t_obs'], np.add.reduceat(M.y, M.k_lim[:-1]))
    np.testing.assert_array_equal(res['site_t_obs'], np.add.reduceat(res['t_obs'], first[:-1]))
    np.testing.assert_allclose(res['site_t_rep_mean'], np.add.reduceat(res['t_rep_mean'], first[:-1]), rtol=1e-13)
    assert np.all((res['p_t'] >= 0) & (res['p_t'] <= 1) & (res['p_t_ge'] >= res['p_t']))
    assert 'draws' not in M.ppc(seed=5)
    assert np.any(M.ppc(seed=6)['t_rep_mean'] != res['t_rep_mean'])
    with pytest.raises(ValueError, match='seed'):
        M.ppc(seed=-1)
    with pytest.raises(ValueError, match='level'):
        M.ppc(level=0.0)


# ------------------------------------------------------------------ two ranks over gloo
RANK_KEYS = KEYS + tuple('site_' + k for k in KEYS[1:]) + ('n', 'extreme')


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
    res = M.ppc(seed=11, level=0.2)
    refused = 0
    try:
        M.ppc(draws=True)
    except ValueError as e:
        refused = int('2 ranks' in str(e))
    np.savez(os.path.join(outdir, 'r%d.npz' % rank), refused=refused, **dict((k, np.asarray(res[k])) for k in RANK_KEYS))
    tdist.barrier()
    tdist.destroy_process_group()


def test_two_ranks_ppc_equals_one_rank(tmp_path):
    """7 groups on 3 sites, sharded 1 + 2 (the sites' records differ in width): every rank checks its own sites with the
    rows' GLOBAL index in the stream, the records are gathered, and both ranks return what one rank returns, bit for
    bit."""
    import torch.multiprocessing as mp
    from oracle.engine_oracle import OracleEngine
    mp.spawn(_worker, args=(2, tph._free_port(), str(tmp_path)), nprocs=2, join=True)
    M, data, Nk, j_ind = tph._groups_master(
        _engine_factory=lambda m, X, y, kl, **g: OracleEngine(m, X, y, kl, nthreads=2, **g))
    M.run(1, verbose=False, seed=3)
    res = M.ppc(seed=11, level=0.2)
    assert np.all(np.isfinite(res['p_t'])) and len(set(M._site_ng)) > 1
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), 'r%d.npz' % r))
        assert int(z['refused']) == 1
        for key in RANK_KEYS:
            np.testing.assert_array_equal(z[key], np.asarray(res[key]), err_msg=key)
