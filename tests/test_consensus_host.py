"""Consensus Monte Carlo (epstan_amd.consensus, the `run_consensus` branch of /root/reference/experiment/fit.py:537-675)
on CPU: the oracle engine stands in for the device, with `pooled_moments` added in NumPy from its `get_draws`; the host
logic -- site priors, partitions, seeds, the two-pass pooling with its all-reduces, the result schema, `fit.main`'s
branches -- is the code under test."""

import os
import socket
import sys

import numpy as np
import pytest

from epstan_amd import fit, models
from epstan_amd.seeds import MAX_UINT
from epstan_amd.util import distribute_groups
from oracle import ep_oracle as eo
from oracle.engine_oracle import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0**-53
CONS_KEYS = {'conf', 'm_s_cons', 'S_s_cons', 'time_s_cons', 'mstepsize_s_cons', 'mrhat_s_cons'}     # fit.py:664-672


class PoolingOracle(OracleEngine):
    """The oracle engine plus HipEngine.pooled_moments, from the draws it holds; records the sampling calls of the
    consensus run (options from the engine's own `sampler_opts`: a dict here)."""
    calls = []

    def sample_batch(self, seeds, opts, k0=0, count=None):
        if isinstance(opts, dict):
            type(self).calls.append((np.array(seeds), dict(opts), self.K))
        return OracleEngine.sample_batch(self, seeds, opts, k0, count)

    def pooled_moments(self, center=None, k0=0, count=None, theta=None, want_scatter=True):
        count = self.K - k0 if count is None else count
        x = np.concatenate([self.get_draws(k) for k in range(k0, k0 + count)], axis=0)
        c = x - (0.0 if center is None else np.asarray(center))
        return x.shape[0], c.sum(axis=0), (np.asfortranarray(c.T.dot(c)) if want_scatter else None)


def factory(model, X, y, k_lim, **groups):
    return PoolingOracle(model, X, y, k_lim, nthreads=2, **groups)


def pooled_bounds(x):
    """Exact (longdouble) mean and covariance of the rows of x and the rounding bounds of ANY float64 summation order:
    |sum_i - exact| <= 2 n u sum|x_i|  and  |scatter_ij - exact| <= 2 (n + 4) u sum |a_i||a_j|, a = x - mean (the factor
    2: the rounding of the centring and the second-order terms), carried to the mean (/ n) and the covariance (/ (n - 1))."""
    n = x.shape[0]
    xl = x.astype(np.longdouble)
    m = xl.sum(axis=0) / n
    a = xl - m
    S = a.T.dot(a) / (n - 1)
    tol_m = 2 * n * U * np.abs(x).sum(axis=0) / n
    aa = np.abs(np.asarray(a, dtype=np.float64))
    tol_S = 2 * (n + 4) * U * aa.T.dot(aa) / (n - 1)
    return np.asarray(m, dtype=np.float64), np.asarray(S, dtype=np.float64), tol_m, tol_S


def reference_draws(model_name, conf, it):
    """The concatenated phi draws of all consensus sites as the reference forms them (fit.py:545-646): every site against
    the prior to the power 1/K, seeds `RandomState(seed_cons).randint(0, MAX_UINT, K)`, sampled by the oracle directly."""
    J, D, K = conf.J, conf.D, conf.K
    model = models.MODELS[model_name](J, D, conf.npg)
    data = model.simulate_data(Sigma_x='rand', rng=conf.seed_data)
    _, _, Q0, r0 = model.get_prior()
    d = Q0.shape[0]
    Om, mu, ok = eo.cavity(np.asfortranarray(Q0 / K), r0 / K, np.zeros((d, d), order='F'), np.zeros(d))
    assert ok
    if K < J:
        Nk, Nj_k, j_ind_k = distribute_groups(J, K, data.Nj)
        k_lim = np.concatenate(([0], np.cumsum(Nk)))
        g_lim = np.concatenate(([0], np.cumsum(data.Nj)))
        eng = OracleEngine(model_name, data.X, data.y, k_lim, nthreads=2, g_cnt=Nj_k, g_lim=g_lim)
    else:
        eng = OracleEngine(model_name + '_sg', data.X, data.y, np.concatenate(([0], np.cumsum(data.Nj))), nthreads=2)
    eng.cav_Om[:] = Om
    eng.cav_mu[:] = mu
    seeds = np.random.RandomState(seed=conf.seed_cons).randint(0, MAX_UINT, size=K)
    stats, _ = eng.sample_batch(seeds, eng.sampler_opts(chains=conf.chains, iter=it, warmup=None, thin=1, init='random'))
    return np.concatenate([eng.get_draws(k) for k in range(K)], axis=0), stats, seeds


def check_against_reference(res, model_name, conf, iters):
    for i, it in enumerate(iters):
        x, stats, _ = reference_draws(model_name, conf, it)
        assert x.shape[0] == conf.K * conf.chains * (it - it // 2)
        m, S, tol_m, tol_S = pooled_bounds(x)
        assert np.all(np.abs(res['m_s_cons'][i] - m) <= tol_m), np.abs(res['m_s_cons'][i] - m) / tol_m
        assert np.all(np.abs(res['S_s_cons'][i] - S) <= tol_S), np.abs(res['S_s_cons'][i] - S) / tol_S
        np.testing.assert_allclose(res['mstepsize_s_cons'][i], stats[:, 0].mean(), rtol=1e-13)
        assert res['mrhat_s_cons'][i] == stats[:, 1].max()
        assert np.isfinite(res['time_s_cons'][i]) and res['time_s_cons'][i] >= 0


@pytest.fixture(scope='module')
def m1b_run(tmp_path_factory):
    """ONE consensus run of m1b, J = K = 4, shared by the tests that read it."""
    out = tmp_path_factory.mktemp('cons')
    conf = fit.configurations(J=4, D=3, K=4, npg=15, run_consensus=True, id='c')
    keep = fit.RES_PATH
    fit.RES_PATH = str(out)
    PoolingOracle.calls = []
    try:
        res = fit.main('m1b', conf, verbose=False, _engine_factory=factory, iters=[40, 60])
    finally:
        fit.RES_PATH = keep
    return conf, res, str(out), list(PoolingOracle.calls)


def test_consensus_result_has_the_reference_schema_and_moments(m1b_run):
    conf, res, out, calls = m1b_run
    d = 4
    assert set(res) == CONS_KEYS
    assert res['m_s_cons'].shape == (2, d) and res['S_s_cons'].shape == (2, d, d)
    for key in ('time_s_cons', 'mstepsize_s_cons', 'mrhat_s_cons'):
        assert res[key].shape == (2,) and np.all(np.isfinite(res[key]))
    saved = np.load(os.path.join(out, 'res_c_m1b_c.npz'), allow_pickle=True)
    assert set(saved.files) == CONS_KEYS
    np.testing.assert_array_equal(saved['S_s_cons'], res['S_s_cons'])
    assert saved['conf'].item()['seed_cons'] == 3
    check_against_reference(res, 'm1b', conf, [40, 60])
    for S in res['S_s_cons']:
        np.testing.assert_array_equal(S, S.T)
        assert np.linalg.eigvalsh(S)[0] > 0


def test_consensus_sampling_calls_use_the_same_seeds_and_start_afresh(m1b_run):
    conf, res, out, calls = m1b_run
    want = np.random.RandomState(seed=3).randint(0, MAX_UINT, size=4)
    assert len(calls) == 2                                     # ONE batched launch per iteration count
    for (seeds, opts, K), it in zip(calls, (40, 60)):
        np.testing.assert_array_equal(seeds, want)
        assert K == 4 and opts['iter'] == it and opts['chains'] == 4 and opts['warmup'] is None and opts['thin'] == 1
        assert opts['init'] == 'random' and not opts['carry']


def test_consensus_iteration_counts():
    from epstan_amd import consensus
    assert consensus.consensus_iters(4, 8) == [50, 100, 500, 1000, 2000, 4000]
    assert consensus.consensus_iters(8, 8) == [50, 100, 500, 1000, 2000, 4000, 6800]
    assert consensus.consensus_iters(8, 8) == consensus.consensus_iters(8, 8)          # no list grows from call to call
    assert all(isinstance(i, int) for i in consensus.consensus_iters(8, 8))


def test_consensus_with_several_groups_per_site():
    conf = fit.configurations(J=6, K=3, D=2, npg=12, chains=2, run_consensus=True, save_res=False)
    res = fit.main('m4b', conf, verbose=False, _engine_factory=factory, iters=[40])
    assert res['m_s_cons'].shape == (1, 6) and res['S_s_cons'].shape == (1, 6, 6)
    check_against_reference(res, 'm4b', conf, [40])


def test_consensus_error_conventions(tmp_path, monkeypatch):
    monkeypatch.setattr(fit, 'RES_PATH', str(tmp_path))
    with pytest.raises(ValueError):
        fit.main('m1b', fit.configurations(J=4, D=3, K=1, npg=15, run_consensus=True), _engine_factory=factory, iters=[40])
    with pytest.raises(NotImplementedError):
        fit.main('m1b', fit.configurations(J=4, D=3, K=8, npg=15, run_consensus=True), _engine_factory=factory, iters=[40])
    for flag in ('run_full', 'run_target', 'run_all'):
        with pytest.raises(NotImplementedError) as ex:
            fit.main('m1b', fit.configurations(J=4, D=3, K=4, npg=15, run_consensus=True, **{flag: True}),
                     _engine_factory=factory, iters=[40])
        assert 'run_full' in str(ex.value) and 'consensus' not in str(ex.value)
    assert not os.listdir(str(tmp_path))


def test_ep_and_consensus_together_return_both_key_sets(tmp_path, monkeypatch, m1b_run):
    monkeypatch.setattr(fit, 'RES_PATH', str(tmp_path))
    kw = dict(J=4, D=3, K=4, npg=15, iter=2, siter=40, run_ep=True, id='b')
    ep = fit.main('m1b', fit.configurations(**kw), verbose=False, _engine_factory=factory)
    both = fit.main('m1b', fit.configurations(run_consensus=True, **kw), verbose=False, _engine_factory=factory, iters=[40, 60])
    assert set(both) == set(ep) | (CONS_KEYS - {'conf'})
    for key in set(ep) - {'conf', 'time_s_ep', 'othertimes'}:               # (clocks differ from run to run)
        np.testing.assert_array_equal(both[key], ep[key])
    for key in CONS_KEYS - {'conf', 'time_s_cons'}:
        np.testing.assert_array_equal(both[key], m1b_run[1][key])
    assert set(os.listdir(str(tmp_path))) == {'res_d_m1b_b.npz', 'res_c_m1b_b.npz'}
    assert set(np.load(os.path.join(str(tmp_path), 'res_d_m1b_b.npz'), allow_pickle=True).files) == set(ep) - {'phi_true'}


# ------------------------------------------------------------------ two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, outdir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['RANK'] = str(rank)
    os.environ['WORLD_SIZE'] = str(world)
    for p in (ROOT, os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as tdist
    from epstan_amd import dist, fit as wfit
    import test_consensus_host as me
    tdist.init_process_group('gloo', rank=rank, world_size=world)
    wfit.RES_PATH = outdir
    conf = wfit.configurations(J=4, D=3, K=4, npg=15, run_consensus=True, id='c')
    res = wfit.main('m1b', conf, verbose=False, _engine_factory=me.factory, iters=[40, 60], comm=dist.TorchComm())
    np.savez(os.path.join(outdir, 'r%d.npz' % rank), sites=[c[2] for c in me.PoolingOracle.calls],
             **dict((k, v) for k, v in res.items() if k != 'conf'))
    tdist.barrier()
    tdist.destroy_process_group()


def test_two_ranks_pool_the_draws_of_all_sites(tmp_path, m1b_run):
    """The sites sharded 2 + 2 over a world-size-2 gloo group: every rank samples its own sites with their GLOBAL seeds
    and the all-reduced sums give the moments of the single-process run, up to the summation order."""
    import torch.multiprocessing as mp
    conf, res, _, _ = m1b_run
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    out = [np.load(os.path.join(str(tmp_path), 'r%d.npz' % r)) for r in range(2)]
    check_against_reference(res, 'm1b', conf, [40, 60])
    for r in out:
        assert list(r['sites']) == [2, 2]                                   # two launches, two local sites each
        check_against_reference(r, 'm1b', conf, [40, 60])
        for key in ('m_s_cons', 'S_s_cons', 'mstepsize_s_cons', 'mrhat_s_cons'):
            np.testing.assert_array_equal(r[key], out[0][key])              # every rank holds the same result
        assert r['mrhat_s_cons'].tolist() == res['mrhat_s_cons'].tolist()
    assert os.path.exists(os.path.join(str(tmp_path), 'res_c_m1b_c.npz'))
