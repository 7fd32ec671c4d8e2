"""k_site_order_stats / k_pooled_count / Master.mix_quantiles on the device: order statistics across draws in device memory
against quantiles.py (NumPy, sorted by key).  Need a real MI355X.

Tolerances.  A name that is a coordinate of the draw (phi, eta, etb, mu_a, mu_b) is selected, never computed: bit-equal.
A transformed name (alpha, beta, sigma*) goes through the device exponential, which differs from libm by ~2e-16
relative: the value at a rank is another function value of the same draw, rtol 1e-12 (plus 1e-15 of the element's largest
draw: alpha = mu_a + eta sigma_a cancels).  Where the host's neighbour in rank lies within test_gpu_named_moments' RTOL =
1e-9 of the selected value the two orders may pick different draws: RTOL there."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from epstan_amd import _lib, fit, models, site_params, quantiles as qt        # noqa: E402
from epstan_amd.engine import HipEngine, MODEL_IDS, is_gauss                  # noqa: E402
from test_gpu_parity import _site_problem, _engine_with_cavity, _group_problem   # noqa: E402
from test_quantiles_host import KINDS, PROBS, adversarial, bits               # noqa: E402

RTOL = 1e-9
COORDS = ('phi', 'eta', 'etb', 'mu_a', 'mu_b')
MAX_DRAWS = 16384                                        # include/epx.h: epx_named_order_stats


def _spec(model):
    return MODEL_IDS[model] % 5, is_gauss(model), model.endswith('_sg')


def _ranks(S):
    return np.unique(np.concatenate([qt.rank_plan(S, PROBS)[0], [0, S - 1]]))


def _bound(x, ranks):
    """Per (rank, element) the bound of the module's docstring from the host's sorted draws x (S, ...)."""
    s = np.sort(x, axis=0)
    n = s.shape[0]
    v = s[ranks]
    shape = (-1,) + (1,) * (x.ndim - 1)
    up = np.where((ranks + 1 < n).reshape(shape), np.abs(s[np.minimum(ranks + 1, n - 1)] - v), np.inf)
    dn = np.where((ranks > 0).reshape(shape), np.abs(v - s[np.maximum(ranks - 1, 0)]), np.inf)
    near = np.minimum(up, dn) <= RTOL * np.abs(v)
    return np.where(near, RTOL, 1e-12) * np.abs(v) + 1e-15 * np.abs(x).max(axis=0)


def _assert_stats(got, x, ranks, name, what):
    """got (R, ...) of the device against the draws x (S, ...) of one name at one site."""
    want = qt.order_stats(x, ranks)
    assert got.shape == want.shape, (what, name)
    if name in COORDS:
        assert bits(got).tolist() == bits(want).tolist(), (what, name)
    else:
        err, tol = np.abs(got - want), _bound(x, ranks)
        print('%s %s: largest error / bound %.3g' % (what, name, (err / tol).max()))
        assert np.all(err <= tol), (what, name)


def _raw_order(eng, names, ranks, theta, k0=0, count=None):
    """The C entry point itself: (n, out (count, L, R)), rows as the library lays them out."""
    count = eng.K - k0 if count is None else count
    ids = np.array([site_params.NAME_IDS[n] for n in names], dtype=np.int32)
    kmax = 0 if eng.g_cnt is None else int(np.argmax(eng.g_cnt))
    L = 0
    for i in ids:
        n = ctypes.c_int()
        _lib.check(eng.lib.epx_named_len(eng.ctx, kmax, int(i), ctypes.byref(n)))
        L += n.value
    ranks = np.ascontiguousarray(ranks, dtype=np.int64)
    out = np.full((count, L, len(ranks)), 7.0)
    S = 0
    if theta is not None:
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        S = theta.shape[1]
    n = ctypes.c_int()
    rc = eng.lib.epx_named_order_stats(eng.ctx, k0, count, ids.ctypes.data_as(_lib.c_int32_p), len(names),
                                       ranks.ctypes.data_as(_lib.c_int64_p), len(ranks), _lib.dptr(theta), S,
                                       _lib.dptr(out), ctypes.byref(n))
    return rc, n.value, out


# ------------------------------------------------------------------ (a) per-site order statistics, injected draws
@pytest.mark.parametrize('model', ['m1b_sg', 'm4b_sg', 'm4a_sg'])
@pytest.mark.parametrize('D', [1, 3, 21])
def test_site_order_stats_match_the_host(model, D):
    K = 5
    X, y, k_lim, _, _, d, P = _site_problem(model, D, 7, 300 + D, K=K)
    eng = HipEngine(model, X, y, k_lim)
    mid, gauss, sg = _spec(model)
    names = site_params.names(mid, gauss)
    for S in (1, 2, 3, 63, 64, 65, 100, 257, 1000):      # the padding and wave-width edges of the sort
        theta = 0.5 * np.random.RandomState(7 * S + D).randn(K, S, P) + 0.3
        ranks = _ranks(S)
        stats = eng.named_order_stats(names, ranks, theta=theta)
        assert len(stats) == K
        for k in range(K):
            draws = site_params.named_draws(mid, D, 1, gauss, sg, theta[k], names)
            for name in names:
                _assert_stats(stats[k][name], draws[name], ranks, name, 'S=%d site %d' % (S, k))
        if S == 100:                                     # a sub-range: the same numbers as the slice of the full call
            sub = eng.named_order_stats(names, ranks, k0=1, count=3, theta=theta[1:4])
            for j in range(3):
                for name in names:
                    assert bits(sub[j][name]).tolist() == bits(stats[1 + j][name]).tolist()
            again = eng.named_order_stats(names, ranks, theta=theta)
            assert all(bits(again[k][nm]).tolist() == bits(stats[k][nm]).tolist() for k in range(K) for nm in names)
    eng.close()


def test_wide_name_list_of_multi_group_sites_and_nan_padding():
    model, D, groups = 'm4b', 21, [[5], [4, 3, 4, 5, 3, 4]]          # all names: 352 elements per row
    S, K = 30, len(groups)
    X, y, k_lim, g_cnt, g_lim, _, _, d = _group_problem(model, D, groups, 23)
    eng = HipEngine(model, X, y, k_lim, g_cnt=g_cnt, g_lim=g_lim)
    mid, gauss, sg = _spec(model)
    names = site_params.names(mid, gauss)
    rng = np.random.RandomState(3)
    theta = np.full((K, S, eng.P), np.nan)                              # NaN behind every site's own coordinates
    for k in range(K):
        theta[k, :, :eng.site_P[k]] = 0.5 * rng.randn(S, eng.site_P[k])
    ranks = _ranks(S)
    stats = eng.named_order_stats(names, ranks, theta=theta)
    for k in range(K):
        draws = site_params.named_draws(mid, D, int(g_cnt[k]), gauss, sg, theta[k, :, :eng.site_P[k]], names)
        for name in names:
            assert np.all(np.isfinite(stats[k][name]))
            _assert_stats(stats[k][name], draws[name], ranks, name, 'site %d' % k)
    rc, n, full = _raw_order(eng, names, ranks, theta)
    assert rc == 0 and n == S and full.shape[1] == 352
    at = 0
    for name in names:                                                  # per-name calls: the same numbers
        one = eng.named_order_stats([name], ranks, theta=theta)
        rc, _, raw = _raw_order(eng, [name], ranks, theta)
        assert rc == 0
        width = raw.shape[1]
        assert bits(raw).tolist() == bits(full[:, at:at + width]).tolist() or np.array_equal(
            raw, full[:, at:at + width], equal_nan=True)
        for k in range(K):
            own = int(np.size(stats[k][name][0]))
            assert bits(one[k][name]).tolist() == bits(stats[k][name]).tolist()
            assert np.array_equal(full[k, at:at + own].T.reshape(stats[k][name].shape), stats[k][name])
            assert np.all(np.isnan(full[k, at + own:at + width]))       # NaN behind the site's own elements
        at += width
    assert at == 352
    eng.close()


# ------------------------------------------------------------------ (b) adversarial values, both routes
def _pooled(eng, names, ranks, theta, k0=0, count=None):
    return qt.select_pooled(lambda shift, prefix: eng.pooled_count_pass(names, shift, prefix, len(ranks), k0=k0,
                                                                        count=count, theta=theta),
                            lambda buf: buf, ranks)


@pytest.mark.parametrize('kind', KINDS + ['nan'])
def test_adversarial_values_both_routes(kind):
    model, D, K, S = 'm4b_sg', 3, 5, 37
    X, y, k_lim, _, _, d, P = _site_problem(model, D, 7, 11, K=K)
    eng = HipEngine(model, X, y, k_lim)
    rng = np.random.RandomState(len(kind))
    src = 'random' if kind == 'nan' else kind
    theta = np.stack([np.stack([adversarial(rng, S, src) for _ in range(P)], axis=1) for _ in range(K)])
    if kind == 'nan':
        theta[2, 5, 3] = np.nan                          # phi[3] = mu_b[1] of site 2, one draw
    names = list(COORDS)
    ranks = _ranks(S)
    stats = eng.named_order_stats(names, ranks, theta=theta)
    for k in range(K):
        want = qt.site_order_stats_host(3, D, 1, False, True, theta[k], names, ranks)
        for name in names:
            nan = np.isnan(want[name])
            assert np.array_equal(np.isnan(stats[k][name]), nan), (k, name)
            assert bits(np.where(nan, 0.0, stats[k][name])).tolist() == bits(np.where(nan, 0.0, want[name])).tolist(), (k, name)
        if kind == 'nan':
            assert np.isnan(want['phi']).sum() == (len(ranks) if k == 2 else 0)
    shared = ['phi', 'mu_a', 'mu_b']
    pr = _ranks(K * S)
    values, n_nan, n = _pooled(eng, shared, pr, theta)
    pool = np.concatenate([np.concatenate([site_params.named_draws(3, D, 1, False, True, theta[k], shared)[nm].reshape(S, -1)
                                           for nm in shared], axis=1) for k in range(K)])
    want = qt.order_stats(pool, pr).T
    nan = np.isnan(want)
    assert n == K * S and n_nan.tolist() == np.isnan(pool).sum(axis=0).tolist()
    assert (n_nan.sum() == 2) == (kind == 'nan')         # phi[3] and mu_b[1] are the same coordinate
    assert np.array_equal(np.isnan(values), nan)
    assert bits(np.where(nan, 0.0, values)).tolist() == bits(np.where(nan, 0.0, want)).tolist()
    eng.close()


# ------------------------------------------------------------------ (c) the pooled passes
@pytest.mark.parametrize('model,names,S,T', [('m4b_sg', ['phi', 'mu_a', 'mu_b'], 37, None), ('m4a_sg', ['phi'], 37, 32),
                                             ('m4b_sg', ['mu_a'], 37, 1), ('m1b_sg', ['phi'], 1000, None)])
def test_pooled_passes_equal_the_host_counts(model, names, S, T):
    D, K = 3, 5
    X, y, k_lim, _, _, d, P = _site_problem(model, D, 7, 13, K=K)
    eng = HipEngine(model, X, y, k_lim)
    mid, gauss, sg = _spec(model)
    theta = 0.5 * np.random.RandomState(S).randn(K, S, P) + 0.3
    theta[:, :, 0] = np.round(theta[:, :, 0], 1) + 0.0   # ties in one coordinate (+ 0.0: no -0.0, which np.sort does not place)
    n = K * S
    ranks = _ranks(n) if T is None else np.unique(np.linspace(0, n - 1, T).astype(np.int64))
    x = [np.concatenate([site_params.named_draws(mid, D, 1, gauss, sg, theta[k], names)[nm].reshape(S, -1) for nm in names],
                        axis=1) for k in range(K)]
    pool = np.concatenate(x)
    shifts = []

    def count_pass(shift, prefix):
        shifts.append(shift)
        got = eng.pooled_count_pass(names, shift, prefix, len(ranks), theta=theta)
        want = qt.count_pass_host(pool, shift, prefix, len(ranks))
        lo = eng.pooled_count_pass(names, shift, prefix, len(ranks), k0=0, count=2, theta=theta[:2])
        hi = eng.pooled_count_pass(names, shift, prefix, len(ranks), k0=2, count=3, theta=theta[2:])
        assert got[0].dtype == np.int64 and got[0].shape == (pool.shape[1], len(ranks), 256)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] == n, shift
        assert np.array_equal(lo[0] + hi[0], want[0]) and np.array_equal(lo[1] + hi[1], want[1]), shift
        assert lo[2] == 2 * S and hi[2] == 3 * S and got[0].sum(axis=2).max() <= n
        if shift == 56:
            assert np.all(got[0].sum(axis=2) == n)       # every draw counts
        return got

    values, n_nan, n_tot = qt.select_pooled(count_pass, lambda buf: buf, ranks)
    assert shifts == [56, 48, 40, 32, 24, 16, 8, 0] and n_tot == n and np.all(n_nan == 0)
    assert bits(values).tolist() == bits(np.sort(pool, axis=0)[ranks].T).tolist()
    eng.close()


def test_pooled_selection_of_transformed_names():
    model, D, K, S = 'm4a_sg', 3, 5, 37
    X, y, k_lim, _, _, d, P = _site_problem(model, D, 7, 17, K=K)
    eng = HipEngine(model, X, y, k_lim)
    theta = 0.5 * np.random.RandomState(4).randn(K, S, P) + 0.3
    names = ['sigma', 'sigma_a', 'sigma_b', 'phi']
    ranks = _ranks(K * S)
    values, _, n = _pooled(eng, names, ranks, theta)
    at = 0
    for name in names:
        pool = np.concatenate([site_params.named_draws(3, D, 1, True, True, theta[k], [name])[name].reshape(S, -1)
                               for k in range(K)])
        _assert_stats(values[at:at + pool.shape[1]].T, pool, ranks, name, 'pooled')
        at += pool.shape[1]
    assert at == values.shape[0] and n == K * S
    eng.close()


# ------------------------------------------------------------------ (d) argument errors: messages, not launches
def test_argument_errors():
    D, K = 3, 2
    X, y, k_lim, Oms, mus, d, P = _site_problem('m4b_sg', D, 7, 5, K=K)
    eng, _, _ = _engine_with_cavity('m4b_sg', X, y, k_lim, Oms, mus)
    with pytest.raises(_lib.EpxError, match='no draws yet'):           # nothing sampled yet
        eng.named_order_stats(['phi'], [0])
    with pytest.raises(_lib.EpxError, match='no draws yet'):
        eng.pooled_count_pass(['phi'], 56, None, 1)
    theta = np.zeros((K, 40, P))
    with pytest.raises(_lib.EpxError, match='at most %d' % MAX_DRAWS):  # one beyond the stated LDS limit
        eng.named_order_stats(['mu_a'], [0], k0=0, count=1, theta=np.zeros((1, MAX_DRAWS + 1, P)))
    assert eng.named_order_stats(['mu_a'], [0, MAX_DRAWS - 1], k0=0, count=1,
                                 theta=np.zeros((1, MAX_DRAWS, P)))[0]['mu_a'].tolist() == [0.0, 0.0]   # the limit itself
    with pytest.raises(_lib.EpxError, match='between 1 and 32 ranks'):
        eng.named_order_stats(['phi'], np.arange(33), theta=np.zeros((K, 64, P)))
    with pytest.raises(_lib.EpxError, match='between 1 and 32 ranks'):
        eng.named_order_stats(['phi'], [], theta=theta)
    with pytest.raises(_lib.EpxError, match=r'rank 40 outside \[0, 40\)'):
        eng.named_order_stats(['phi'], [3, 40], theta=theta)
    with pytest.raises(_lib.EpxError, match='rank -1 outside'):
        eng.named_order_stats(['phi'], [-1, 3], theta=theta)
    with pytest.raises(_lib.EpxError, match='ascending and distinct'):
        eng.named_order_stats(['phi'], [3, 3], theta=theta)
    with pytest.raises(_lib.EpxError, match='not defined'):
        eng.named_order_stats(['sigma'], [3], theta=theta)
    with pytest.raises(_lib.EpxError, match='shift = 7'):
        eng.pooled_count_pass(['phi'], 7, np.zeros((d, 1), dtype=np.uint64), 1, theta=theta)
    with pytest.raises(_lib.EpxError, match='between 1 and 32 targets'):
        eng.pooled_count_pass(['phi'], 56, None, 33, theta=theta)
    with pytest.raises(ValueError, match='prefix'):
        eng.pooled_count_pass(['phi'], 48, np.zeros((d, 2), dtype=np.uint64), 1, theta=theta)
    eng.close()
    X, y, k_lim, g_cnt, g_lim, _, _, d = _group_problem('m4b', D, [[9], [8, 7, 9], [10, 6]], 23)
    eng = HipEngine('m4b', X, y, k_lim, g_cnt=g_cnt, g_lim=g_lim)
    theta = np.zeros((3, 8, eng.P))
    with pytest.raises(_lib.EpxError, match='equal lengths'):          # the sites hold 1, 3 and 2 groups
        eng.pooled_count_pass(['alpha'], 56, None, 1, theta=theta)
    hist, n_nan, n = eng.pooled_count_pass(['phi'], 56, None, 1, theta=theta)        # what every site holds alike: fine
    assert n == 24 and hist.shape == (d, 1, 256) and np.all(hist[:, 0, 0x80] == 24) and hist.sum() == 24 * d
    eng.close()


# ------------------------------------------------------------------ (e) the sampler's draws, Master.mix_quantiles on the device
def _quantile_bound(x, probs):
    """(want, bound) of the quantiles of the draws x (n, ...): the order statistics' bounds carried through
    x_(i) + g (x_(i+1) - x_(i)), whose error is a mean of the two ends' errors, plus its rounding."""
    ranks, plan = qt.rank_plan(x.shape[0], probs)
    want = qt.interpolate(qt.order_stats(x, ranks), ranks, plan)
    b = _bound(x, ranks)
    at = [int(np.searchsorted(ranks, i)) for i, _ in plan]
    bound = np.stack([np.maximum(b[a], b[min(a + 1, len(ranks) - 1)]) for a in at]) + 4 * np.spacing(np.abs(x).max(axis=0))
    return want, bound


@pytest.mark.parametrize('J,K', [(4, 4), (5, 3)])
def test_master_mix_quantiles_on_the_device(J, K):
    D = 3
    conf = fit.configurations(J=J, D=D, K=K, npg=30, siter=40, run_ep=True, damp=0.4)
    M = fit.main('m4b', conf, ret_master=True)
    assert isinstance(M.engine, HipEngine)
    with pytest.raises(RuntimeError, match='at least one iteration'):
        M.mix_quantiles('phi')
    assert M.run(2, verbose=False, calc_moments=False, seed=5) == 0
    multi = K < J
    mid, gauss, sg = _spec(M.model_name)
    pnames, pshapes, phiers = models.m4b(J, D, 30).get_param_definitions()
    pmaps = fit._create_pmaps(phiers, J, K, M._site_ng if multi else None)
    names = list(pnames) + ['phi', 'sigma_a', 'sigma_b', 'mu_a', 'mu_b']

    def named(k):
        theta = np.ascontiguousarray(M.engine.get_draws(k, all_params=True))
        return site_params.named_draws(mid, D, int(M._site_ng[k]), gauss, sg,
                                       theta[:, :M.engine.site_P[k]] if multi else theta, names)
    draws = [named(k) for k in range(K)]
    S = M.engine.num_draws()
    ranks = _ranks(S)
    stats = M.engine.named_order_stats(names, ranks)                   # the order statistics themselves
    for k in range(K):
        for name in names:
            _assert_stats(stats[k][name], draws[k][name], ranks, name, 'site %d' % k)
    res = M.mix_quantiles(pnames, smap=pmaps, param_shapes=pshapes)
    for name, shape, mp, q in zip(pnames, pshapes, pmaps, res):
        assert q.shape == (5,) + tuple(shape) and np.all(np.isfinite(q))
        for k in range(K):
            want, bound = _quantile_bound(draws[k][name], PROBS)
            got = q[(slice(None),) + (mp[k] if isinstance(mp[k], tuple) else (mp[k],))]
            assert np.all(np.abs(got - want) <= bound), (name, k)
            np.testing.assert_allclose(got, np.quantile(draws[k][name], PROBS, axis=0, method='linear'), rtol=RTOL,
                                       atol=1e-12 * np.abs(draws[k][name]).max())
        assert np.all(q[1] <= q[2]) and np.all(q[2] <= q[3])            # the 50 % row lies between the 25 % and 75 % rows
    shared = ['phi', 'sigma_a', 'sigma_b', 'mu_a', 'mu_b']
    res = M.mix_quantiles(shared)
    for name, q in zip(shared, res):
        pool = np.concatenate([draws[k][name] for k in range(K)])
        want, bound = _quantile_bound(pool, PROBS)
        print('%s: pooled quantiles, largest error / bound %.3g' % (name, (np.abs(q - want) / bound).max()))
        assert q.shape == want.shape and np.all(np.abs(q - want) <= bound), name
        assert np.all(q[1] <= q[2]) and np.all(q[2] <= q[3])
    one = M.mix_quantiles('mu_a', probs=[0.5])
    assert one.shape == (1,) and bits(one).tolist() == bits(res[3][2:3]).tolist()
