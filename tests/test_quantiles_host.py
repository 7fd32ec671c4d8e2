"""`quantiles.py` and `Master.mix_quantiles` on the CPU: the rank plan and the interpolation against np.quantile, the
selection by counting over two shards against np.sort bit for bit on adversarial values, NaN containment, and
`Master.mix_quantiles`' bookkeeping with the oracle standing in for the device engine, on one rank and on two over gloo."""

import os
import sys

import numpy as np
import pytest

from epstan_amd import fit, models, quantiles as qt, site_params

import test_predict_host as tph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def adversarial(rng, n, which):
    """(n,) draws that stress an order by key: ties, neighbours 1 ulp apart, signed zeros, infinities, denormals."""
    if which == 'random':
        return rng.randn(n) * 10.0 ** rng.randint(-3, 4, n)
    if which == 'tied':
        return np.round(rng.randn(n), 1)
    if which == 'ulp':
        return 1.0 + rng.randint(0, max(n // 2, 2), n) * 2.0 ** -52
    if which == 'zeros_infs':
        return rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 5e-324, -5e-324]), n)
    assert which == 'denormal'
    return rng.randint(-1000, 1000, n) * 5e-324 * rng.choice([1.0, 2.0 ** 30], n)


KINDS = ['random', 'tied', 'ulp', 'zeros_infs', 'denormal']


# ------------------------------------------------------------------ the key
def test_key_orders_doubles_and_inverts_bit_for_bit():
    x = np.array([-np.inf, -1e308, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1.0 + 2.0 ** -52, 1e308, np.inf])
    k = qt.key_of(x)
    assert k.dtype == np.uint64 and np.all(k[1:] > k[:-1])
    assert bits(qt.value_of(k)).tolist() == bits(x).tolist()
    rng = np.random.RandomState(0)
    raw = rng.randint(0, 2 ** 62, 1000).astype(np.uint64) * np.uint64(4) + rng.randint(0, 4, 1000).astype(np.uint64)
    assert qt.key_of(raw.view(np.float64)).tolist() != raw.tolist()
    assert bits(qt.value_of(qt.key_of(raw.view(np.float64)))).tolist() == raw.tolist()


# ------------------------------------------------------------------ rank_plan / interpolate against np.quantile
@pytest.mark.parametrize('n', [1, 2, 3, 64, 65, 1000])
def test_rank_plan_and_interpolate_against_numpy(n):
    probs = [0.0, 0.025, 1.0 / 3.0, 0.5, 0.975, 1.0]
    rng = np.random.RandomState(n)
    x = rng.randn(n, 7) * np.array([1e-3, 1.0, 1.0, 30.0, 1e6, 1.0, 1.0]) + np.array([0, 0, 5.0, 0, 0, -1e3, 1e-9])
    ranks, plan = qt.rank_plan(n, probs)
    assert ranks.dtype == np.int64 and np.all(np.diff(ranks) > 0) and ranks[0] >= 0 and ranks[-1] < n
    assert len(plan) == len(probs) and len(ranks) <= 2 * len(probs)
    for (i, g), p in zip(plan, probs):
        assert 0 <= i <= max(n - 2, 0) and 0.0 <= g <= 1.0
        if n > 1:
            assert i in ranks and i + 1 in ranks and abs(i + g - p * (n - 1)) < 1e-9
    stats = qt.order_stats(x, ranks)
    assert bits(stats).tolist() == bits(np.sort(x, axis=0)[ranks]).tolist()
    got = qt.interpolate(stats, ranks, plan)
    want = np.quantile(x, probs, axis=0, method='linear')
    tol = 4 * np.spacing(np.abs(x).max(axis=0))          # 4 ulp of max|x|: the same formula up to NumPy's lerp branch
    err = np.abs(got - want)
    print('n = %d: largest error %.3g ulp of max|x|' % (n, (err / (tol / 4)).max()))
    assert got.shape == (len(probs), 7) and np.all(err <= tol)
    assert bits(got[0]).tolist() == bits(x.min(axis=0)).tolist()          # p = 0: x_(0) + 0 (x_(1) - x_(0))


def test_rank_plan_refuses_bad_probabilities_and_too_many_ranks():
    for bad in ([-0.1], [1.0000001], [0.5, np.nan], [], [[0.5]]):
        with pytest.raises(ValueError, match='probs'):
            qt.rank_plan(10, bad)
    with pytest.raises(ValueError, match='at least one draw'):
        qt.rank_plan(0, [0.5])
    qt.rank_plan(10 ** 6, np.linspace(0.01, 0.99, 16))
    with pytest.raises(ValueError, match='at most 32'):
        qt.rank_plan(10 ** 6, np.linspace(0.01, 0.99, 17))
    r, plan = qt.rank_plan(1, [0.0, 0.3, 1.0])
    assert r.tolist() == [0] and plan == [(0, 0.0)] * 3
    assert qt.interpolate(np.array([[np.inf, 2.0]]), r, plan).tolist() == [[np.inf, 2.0]] * 3     # n = 1: x_(0) itself


# ------------------------------------------------------------------ selection by counting, two unequal shards
def _select_two_shards(x, ranks, cut):
    """select_pooled over the shards x[:cut], x[cut:] (n, L): each pass counts per shard, the 'all-reduce' adds them."""
    shards = [x[:cut], x[cut:]]
    calls = []

    def count_pass(shift, prefix):
        calls.append(shift)
        parts = [qt.count_pass_host(s, shift, prefix, len(ranks)) for s in shards]
        count_pass.other = parts[1]
        return parts[0]

    def allreduce_sum(buf):
        h, nn, n = count_pass.other
        assert buf.dtype == np.float64
        return buf + np.concatenate([h.reshape(-1), nn, [n]]).astype(np.float64)

    out = qt.select_pooled(count_pass, allreduce_sum, ranks)
    assert calls == [56, 48, 40, 32, 24, 16, 8, 0]
    return out


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', [1, 2, 3, 37, 257, 1000])
def test_select_pooled_equals_sort_bit_for_bit(kind, n):
    rng = np.random.RandomState(1000 + n)
    x = np.stack([adversarial(rng, n, kind) for _ in range(3)], axis=1)
    ranks = np.unique(np.concatenate([qt.rank_plan(n, PROBS)[0], [0, n - 1]]))
    values, n_nan, n_tot = _select_two_shards(x, ranks, n // 3)
    assert n_tot == n and np.all(n_nan == 0) and values.shape == (3, len(ranks))
    want = np.take_along_axis(x, np.argsort(qt.key_of(x), axis=0, kind='stable'), axis=0)[ranks].T
    assert bits(values).tolist() == bits(want).tolist()
    if kind not in ('zeros_infs',):                          # (np.sort does not order -0.0 before +0.0)
        assert np.array_equal(values, np.sort(x, axis=0)[ranks].T)
    assert np.array_equal(values.T, qt.order_stats(x, ranks), equal_nan=True)


def test_signed_zeros_and_infinities_are_ordered_by_key():
    x = np.array([0.0, -0.0, np.inf, -np.inf, -0.0, 0.0, 1.0])[:, None]
    values, _, _ = _select_two_shards(x, np.arange(7), 2)
    assert bits(values[0]).tolist() == bits(np.array([-np.inf, -0.0, -0.0, 0.0, 0.0, 1.0, np.inf])).tolist()


def test_a_nan_makes_its_own_element_nan_and_no_other():
    rng = np.random.RandomState(5)
    x = rng.randn(50, 4)
    ranks, plan = qt.rank_plan(50, PROBS)
    clean = _select_two_shards(x, ranks, 20)[0]
    bad = x.copy()
    bad[31, 2] = np.nan
    values, n_nan, n = _select_two_shards(bad, ranks, 20)
    assert n_nan.tolist() == [0, 0, 1, 0] and n == 50
    assert np.all(np.isnan(values[2])) and bits(values[[0, 1, 3]]).tolist() == bits(clean[[0, 1, 3]]).tolist()
    stats = qt.order_stats(bad, ranks)
    assert np.all(np.isnan(stats[:, 2])) and bits(stats[:, [0, 1, 3]]).tolist() == bits(clean[[0, 1, 3]].T).tolist()
    q = qt.interpolate(stats, ranks, plan)
    assert np.all(np.isnan(q[:, 2])) and np.all(np.isfinite(q[:, [0, 1, 3]]))
    with pytest.raises(ValueError, match='rank outside'):
        _select_two_shards(x, [50], 20)
    with pytest.raises(ValueError, match='rank outside'):
        qt.order_stats(x, [50])


def test_site_quantiles_host_forms_the_named_parameters():
    D, S, ng = 3, 41, 2
    P = site_params.layout(3, D, ng, False)[1] + ng * (1 + D)
    theta = 0.5 * np.random.RandomState(2).randn(S, P) + 0.3
    names = site_params.names(3, False)
    got = qt.site_quantiles_host(3, D, ng, False, False, theta, names, PROBS)
    draws = site_params.named_draws(3, D, ng, False, False, theta, names)
    for name in names:
        want = np.quantile(draws[name], PROBS, axis=0, method='linear')
        assert got[name].shape == want.shape == (5,) + draws[name].shape[1:]
        np.testing.assert_allclose(got[name], want, rtol=0, atol=4 * np.spacing(np.abs(draws[name]).max()))


# ------------------------------------------------------------------ Master.mix_quantiles
def _named(M, k, names):
    mid, gauss, sg = M._site_spec()
    theta = np.ascontiguousarray(M.engine.get_draws(k, all_params=True))
    return site_params.named_draws(mid, M.D, int(M._site_ng[k]), gauss, sg, theta, names)


def _close(got, want, draws):
    np.testing.assert_allclose(got, want, rtol=0, atol=4 * np.spacing(np.abs(draws).max()))


def test_master_mix_quantiles_single_group():
    M, data = tph._sg_master()
    with pytest.raises(RuntimeError, match='at least one iteration'):
        M.mix_quantiles('phi')
    assert M.run(1, verbose=False, calc_moments=False, seed=2) == M.INFO_OK
    J = K = 4
    pnames, pshapes, phiers = models.m4b(J, 2, 15).get_param_definitions()
    pmaps = fit._create_pmaps(phiers, J, K, None)
    res = M.mix_quantiles(pnames, smap=pmaps, param_shapes=pshapes)
    assert isinstance(res, list) and len(res) == len(pnames)
    for name, shape, q in zip(pnames, pshapes, res):
        assert q.shape == (5,) + tuple(shape)
        for k in range(K):
            x = _named(M, k, [name])[name]
            _close(q[:, k], np.quantile(x, PROBS, axis=0, method='linear'), x)
        assert np.all(q[1] <= q[2]) and np.all(q[2] <= q[3])
    # parameters every site holds: the pool of all sites' draws
    shared = ['phi', 'sigma_a', 'mu_b', 'sigma_b', 'mu_a']
    res = M.mix_quantiles(shared, probs=[0.0, 0.1, 0.5, 1.0])
    for name, q in zip(shared, res):
        pool = np.concatenate([_named(M, k, [name])[name] for k in range(K)])
        assert q.shape == (4,) + pool.shape[1:] and pool.shape[0] == 320
        _close(q, np.quantile(pool, [0.0, 0.1, 0.5, 1.0], axis=0, method='linear'), pool)
        assert bits(q[0]).tolist() == bits(pool.min(axis=0)).tolist()
    one = M.mix_quantiles('sigma_a', probs=[0.0, 0.1, 0.5, 1.0])
    assert isinstance(one, np.ndarray) and one.shape == (4,) and np.array_equal(one, res[1])
    mixed = M.mix_quantiles(['phi', 'alpha'], smap=[None, pmaps[0]], param_shapes=[None, pshapes[0]])
    assert mixed[0].shape == (5, 6) and mixed[1].shape == (5, 4)

    # ---- refusals
    with pytest.raises(ValueError, match='probs'):
        M.mix_quantiles('phi', probs=[0.5, 1.5])
    with pytest.raises(ValueError, match='every site has to hold the whole parameter|not defined'):
        M.mix_quantiles('gamma')
    with pytest.raises(ValueError, match='param_shapes'):
        M.mix_quantiles('alpha', smap=pmaps[0])
    with pytest.raises(ValueError, match='one index per site'):
        M.mix_quantiles('alpha', smap=list(range(3)), param_shapes=(4,))
    with pytest.raises(ValueError, match='several sites'):
        M.mix_quantiles('alpha', smap=[0, 1, 1, 2], param_shapes=(3,))
    with pytest.raises(ValueError, match='does not fill'):
        M.mix_quantiles('alpha', smap=[0, 1, 2, 3], param_shapes=(5,))

    def from_cavity(data, stan_params):                  # draws of phi alone, as an injector gives them
        z = np.random.RandomState(stan_params['seed'] % 1000).randn(80, 6)
        return data['mu_phi'] + np.linalg.solve(np.linalg.cholesky(data['Omega_phi']).T, z.T).T
    M._sample_injector = from_cavity
    M.run(1, verbose=False, seed=3)
    with pytest.raises(RuntimeError, match='injected'):
        M.mix_quantiles('phi')


def _groups_case():
    """m4b, 7 groups on 3 sites of [[3], [2], [2]] groups: parameters, shapes and maps as fit.main builds them."""
    pnames, pshapes, phiers = models.m4b(7, 2, 25).get_param_definitions()
    return pnames, pshapes, phiers


def _check_groups(M, res, pnames, pshapes, pmaps):
    for name, shape, mp, q in zip(pnames, pshapes, pmaps, res):
        assert q.shape == (5,) + tuple(shape)
        for k in range(M.K):
            x = _named(M, k, [name])[name]
            _close(q[(slice(None),) + (mp[k] if isinstance(mp[k], tuple) else (mp[k],))],
                   np.quantile(x, PROBS, axis=0, method='linear'), x)
        assert np.all(q[1] <= q[2]) and np.all(q[2] <= q[3])


def _uneven_groups_master(groups=((9,), (8, 7, 9), (10, 6)), D=3):
    """`m4b` on sites that hold 1, 3 and 2 groups of the given row counts."""
    from epstan_amd.method import Master
    J = sum(len(g) for g in groups)
    rng = np.random.RandomState(23)
    N = sum(sum(g) for g in groups)
    X = rng.randn(N, D)
    y = (rng.rand(N) < 1.0 / (1.0 + np.exp(-X.dot(0.5 * rng.randn(D)) - 0.3))).astype(np.int64)
    _, _, Q0, r0 = models.m4b(J, D, 9).get_prior()
    Nk = np.array([sum(g) for g in groups])
    Nj_k = np.array([len(g) for g in groups])
    j_ind = np.concatenate([np.repeat(np.arange(len(g)), g) for g in groups]) + 1
    M = Master('m4b', X, y, site_sizes=Nk, A_k={'J': Nj_k}, A_n={'j_ind': j_ind}, prior={'Q': Q0, 'r': r0}, chains=4,
               iter=40, df0=0.4, _engine_factory=tph.factory)
    return M, J, D


def test_master_mix_quantiles_with_several_groups_per_site():
    M, J, D = _uneven_groups_master()                    # 6 groups on 3 sites: 1 + 3 + 2
    M.run(1, verbose=False, seed=3)
    assert M._site_ng.tolist() == [1, 3, 2]
    pnames, pshapes, phiers = models.m4b(J, D, 9).get_param_definitions()
    pmaps = fit._create_pmaps(phiers, J, 3, M._site_ng)
    res = M.mix_quantiles(pnames, smap=pmaps, param_shapes=pshapes)
    _check_groups(M, res, pnames, pshapes, pmaps)
    phi = M.mix_quantiles('phi')
    pool = np.concatenate([_named(M, k, ['phi'])['phi'] for k in range(3)])
    _close(phi, np.quantile(pool, PROBS, axis=0, method='linear'), pool)
    with pytest.raises(ValueError, match='every site has to hold the whole parameter'):
        M.mix_quantiles('alpha')                         # the sites hold different groups: no pool
    overlap = [slice(0, 1), slice(1, 4), slice(3, 5)]    # group 3 twice, group 5 never
    with pytest.raises(ValueError, match='several sites|does not fill'):
        M.mix_quantiles('alpha', smap=overlap, param_shapes=(J,))
    with pytest.raises(ValueError, match='several sites'):
        M.mix_quantiles('alpha', smap=[slice(0, 1), slice(1, 4), slice(2, 4)], param_shapes=(4,))
    with pytest.raises(ValueError, match='one index per site'):
        M.mix_quantiles('alpha', smap=pmaps[0][:2], param_shapes=(J,))
    with pytest.raises(ValueError, match='does not fill'):
        M.mix_quantiles('alpha', smap=pmaps[0], param_shapes=(J + 1,))


# ------------------------------------------------------------------ two ranks over gloo
def _both_routes(M):
    pnames, pshapes, phiers = _groups_case()
    pmaps = fit._create_pmaps(phiers, 7, 3, M._site_ng)
    res = M.mix_quantiles(pnames, smap=pmaps, param_shapes=pshapes)
    pooled = M.mix_quantiles(['phi', 'sigma_a', 'sigma_b'], probs=[0.0, 0.025, 0.5, 0.975, 1.0])
    return dict(alpha=res[0], beta=res[1], phi=pooled[0], sigma_a=pooled[1], sigma_b=pooled[2])


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
    import test_quantiles_host as mine
    tdist.init_process_group('gloo', rank=rank, world_size=world)
    fac = lambda m, X, y, kl, **g: OracleEngine(m, X, y, kl, nthreads=2, **g)
    M, data, Nk, j_ind = me._groups_master(comm=dist.TorchComm(), _engine_factory=fac)
    M.run(1, verbose=False, seed=3)
    np.savez(os.path.join(outdir, 'r%d.npz' % rank), **mine._both_routes(M))
    tdist.barrier()
    tdist.destroy_process_group()


def test_two_ranks_quantiles_equal_one_rank(tmp_path):
    """7 groups on 3 sites, sharded 1 + 2: the per-site order statistics are gathered, the pooled ones selected from counts
    summed over the ranks, and both ranks return what one rank returns, bit for bit."""
    import torch.multiprocessing as mp
    from oracle.engine_oracle import OracleEngine
    mp.spawn(_worker, args=(2, tph._free_port(), str(tmp_path)), nprocs=2, join=True)
    M, data, Nk, j_ind = tph._groups_master(
        _engine_factory=lambda m, X, y, kl, **g: OracleEngine(m, X, y, kl, nthreads=2, **g))
    M.run(1, verbose=False, seed=3)
    res = _both_routes(M)
    assert all(np.all(np.isfinite(v)) for v in res.values())
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), 'r%d.npz' % r))
        for key, want in res.items():
            assert bits(z[key]).tolist() == bits(want).tolist(), key
