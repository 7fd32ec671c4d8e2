"""predict_quantiles.py, the NumPy statement of the order statistics across draws of new rows (include/epx.h, enum
epx_pred_order), and `Master.predict_quantiles` on the CPU: the statement against np.quantile on a linear predictor built
by explicit loops over groups, the replicates' stream, `Master.predict_quantiles`' bookkeeping (rows by site in either
description, the caller's row order, every refusal) with the oracle standing in for the device engine, the resolver, and
the row collective on a two-rank stub."""

import inspect

import numpy as np
import pytest

from epstan_amd import draw_queries as dq, fit, newgroup, ppc, predict_quantiles as pq, quantiles, site_params
from epstan_amd.engine import HipEngine
from oracle.engine_oracle import OracleEngine

PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)


def factory(model, X, y, k_lim, **groups):
    return OracleEngine(model, X, y, k_lim, **groups)


# ------------------------------------------------------------------ the host statement
def _loop_f(mid, D, ng, gauss, theta, Xn, group):
    """f (S, n) group by group, the coefficients straight from the Stan programs' `transformed parameters`."""
    o = 1 if gauss else 0
    S, n = theta.shape[0], Xn.shape[0]
    f = np.empty((S, n))
    for g in range(ng):
        rows = np.nonzero(group == g)[0]
        if mid == 0:                                     # phi = [log sigma_a, beta]
            d = o + 1 + D
            alpha, beta = theta[:, d + g] * np.exp(theta[:, o]), theta[:, o + 1:o + 1 + D]
        else:                                            # phi = [mu_a, log sigma_a, mu_b (D), log sigma_b (D)]
            d = o + 2 + 2 * D
            etb = theta[:, d + ng + g * D:d + ng + (g + 1) * D]
            alpha = theta[:, o] + theta[:, d + g] * np.exp(theta[:, o + 1])
            beta = theta[:, o + 2:o + 2 + D] + etb * np.exp(theta[:, o + 2 + D:o + 2 + 2 * D])
        f[:, rows] = alpha[:, None] + beta.dot(Xn[rows].T)
    return f


def _problem(mid, gauss, ng, D, S, n, seed):
    rng = np.random.RandomState(seed)
    P = site_params.layout(mid, D, ng, gauss)[1] + ng * (1 + (D if mid else 0))
    return 0.5 * rng.randn(S, P) + 0.3, 1.5 * rng.randn(n, D), np.sort(rng.randint(0, ng, n))


CASES = [(0, False, 1), (3, False, 1), (4, False, 1), (3, True, 1), (3, False, 3), (0, False, 2)]
IDS = ['m1b_sg', 'm4b_sg', 'm5b_sg', 'm4a_sg', 'm4b', 'm1b']


@pytest.mark.parametrize('mid,gauss,ng', CASES, ids=IDS)
@pytest.mark.parametrize('S', [1, 2, 23, 100])
def test_host_statement_against_np_quantile(mid, gauss, ng, S):
    D, n = 3, 11
    theta, Xn, group = _problem(mid, gauss, ng, D, S, n, 100 * mid + 10 * ng + S)
    f = _loop_f(mid, D, ng, gauss, theta, Xn, group)
    np.testing.assert_allclose(site_params.linear_predictor(mid, D, ng, gauss, theta, Xn, group), f, rtol=1e-13, atol=1e-14)
    ranks, plan = quantiles.rank_plan(S, PROBS)
    stats = pq.predict_order_stats_host(mid, D, [ng], gauss, [theta], Xn, [0, n], ranks, group if ng > 1 else None)
    assert stats.shape == (n, ranks.size) and np.all(np.diff(stats, axis=1) >= 0)
    got = pq.quantiles_of(stats, ranks, plan, False)
    lp = site_params.linear_predictor(mid, D, ng, gauss, theta, Xn, group)
    exp = np.quantile(lp, PROBS, axis=0, method='linear')
    assert got.shape == (len(PROBS), n)
    np.testing.assert_allclose(got, exp, rtol=1e-13)
    np.testing.assert_allclose(got, np.quantile(f, PROBS, axis=0, method='linear'), rtol=1e-13)      # the independent f
    # through the sigmoid: the quantiles of sigmoid(f), the map being monotone
    got_s = pq.quantiles_of(stats, ranks, plan, True)
    np.testing.assert_allclose(got_s, np.quantile(pq.stable_sigmoid(lp), PROBS, axis=0, method='linear'), rtol=1e-13)


def test_host_statement_sites_nan_and_the_wider_type():
    """Two sites with their own draws and limits, an empty site between them; a NaN draw makes that site's rows NaN at
    every rank and no other; the longdouble evaluation agrees with the float64 one to rounding."""
    D, S = 2, 9
    th0, X0, _ = _problem(3, True, 1, D, S, 4, 1)
    th1, X1, _ = _problem(3, True, 1, D, S, 3, 2)
    Xn, lim, ranks = np.concatenate((X0, X1)), [0, 4, 4, 7], np.arange(S)
    out = pq.predict_order_stats_host(3, D, [1, 1, 1], True, [th0, th0, th1], Xn, lim, ranks)
    np.testing.assert_array_equal(out[:4], np.sort(site_params.linear_predictor(3, D, 1, True, th0, X0, None), axis=0).T)
    np.testing.assert_array_equal(out[4:], np.sort(site_params.linear_predictor(3, D, 1, True, th1, X1, None), axis=0).T)
    bad = th1.copy()
    bad[5, 1] = np.nan                                   # mu_a of one draw
    out2 = pq.predict_order_stats_host(3, D, [1, 1, 1], True, [th0, th0, bad], Xn, lim, ranks)
    assert np.all(np.isnan(out2[4:]))
    np.testing.assert_array_equal(out2[:4], out[:4])
    for what in ('f', 'yrep'):
        a = pq.predict_order_stats_host(3, D, [1, 1, 1], True, [th0, th0, th1], Xn, lim, ranks, what=what, seed=5)
        b = pq.predict_order_stats_host(3, D, [1, 1, 1], True, [th0, th0, th1], Xn, lim, ranks, what=what, seed=5,
                                        dtype=np.longdouble)
        np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-14)


def test_replicates_follow_the_stream_of_their_kind_and_row_id():
    """v = f + exp(phi[0]) z with z the normal of (seed, row_id, draw) at kind 9: rebuilt here cell by cell from the
    stream's uniforms; another kind, seed or row_id gives other replicates, the row order and the other rows do not."""
    D, S, n, seed = 2, 6, 5, 12345678901234567
    theta, Xn, _ = _problem(3, True, 1, D, S, n, 3)
    ids = np.array([7, 2 ** 32 - 1, 0, 2 ** 31, 12])
    assert pq.K_PRED_REP == 9 and pq.K_PRED_REP not in (ppc.K_PPC, newgroup.K_NEWGROUP)
    v = pq.site_values(3, D, 1, True, theta, Xn, None, 'yrep', seed, ids)
    f = site_params.linear_predictor(3, D, 1, True, theta, Xn, None)
    key = newgroup.make_key(seed, 0)
    for i, e in enumerate(ids):
        e32 = int(np.array(e).astype(np.uint32).view(np.int32))
        a = (e32 >> 1) & 0xFFFFFFFF
        for s in range(S):
            u1, u2 = newgroup.rng_u2(key, np.uint64(s), 9, np.uint64(a), 0)
            rad, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586476925286766559 * u2
            z = rad * (np.sin(ang) if e & 1 else np.cos(ang))
            assert v[s, i] == f[s, i] + np.exp(theta[s, 0]) * z
    perm = np.array([3, 0, 4, 1, 2])
    np.testing.assert_array_equal(pq.site_values(3, D, 1, True, theta, Xn[perm], None, 'yrep', seed, ids[perm]), v[:, perm])
    np.testing.assert_array_equal(pq.site_values(3, D, 1, True, theta, Xn[:2], None, 'yrep', seed, ids[:2]), v[:, :2])
    assert np.all(pq.site_values(3, D, 1, True, theta, Xn, None, 'yrep', seed + 1, ids) != v)
    assert np.all(pq.site_values(3, D, 1, True, theta, Xn, None, 'yrep', seed, ids + np.array([1, -1, 1, 1, 1])) != v)
    np.testing.assert_array_equal(ppc.replicate_normals(seed, ids, S), ppc.replicate_normals(seed, ids, S, kind=ppc.K_PPC))
    assert np.all(ppc.replicate_normals(seed, ids, S, kind=9) != ppc.replicate_normals(seed, ids, S))
    with pytest.raises(ValueError, match='Gaussian family only'):
        pq.site_values(3, D, 1, False, theta[:, 1:], Xn, None, 'yrep', seed, ids)
    with pytest.raises(ValueError, match='what'):
        pq.site_values(3, D, 1, True, theta, Xn, None, 'mean', seed, ids)
    with pytest.raises(ValueError, match='2\\^32'):
        pq.site_values(3, D, 1, True, theta, Xn, None, 'yrep', seed, ids + 1)


# ------------------------------------------------------------------ Master.predict_quantiles
def _master(name, J, K):
    conf = fit.configurations(J=J, D=2, K=K, npg=12, iter=1, siter=40, chains=4, run_ep=True, save_res=False)
    return fit.main(name, conf, ret_master=True, verbose=False, _engine_factory=factory)


def _f_by_site(M, Xs, cnt, group):
    """f (S, n) of rows ordered by site, from the engine's downloaded draws."""
    mid, gauss, _ = M._site_spec()
    lim = np.concatenate(([0], np.cumsum(cnt)))
    return np.concatenate([site_params.linear_predictor(
        mid, M.D, int(M._site_ng[k]), gauss, M.engine.get_draws(k, all_params=True), Xs[lim[k]:lim[k + 1]],
        None if group is None else group[lim[k]:lim[k + 1]]) for k in range(M.K)], axis=1)


def test_master_quantiles_linear_and_mean_by_site_sizes_and_shuffled_site_ind():
    M = _master('m4b', 4, 4)                             # one group per site: m4b_sg
    rng = np.random.RandomState(4)
    cnt = np.array([5, 0, 7, 3])                         # a site without new rows
    n = int(cnt.sum())
    Xs = rng.randn(n, 2)
    with pytest.raises(RuntimeError, match='at least one iteration'):
        M.predict_quantiles(Xs, site_sizes=cnt)
    M.run(1, verbose=False, seed=2)
    f = _f_by_site(M, Xs, cnt, None)
    assert f.shape == (80, n)
    lin = M.predict_quantiles(Xs, site_sizes=cnt, scale='linear')
    assert set(lin) == {'quantiles', 'probs', 'scale', 'n'} and lin['n'] == 80 and lin['scale'] == 'linear'
    np.testing.assert_array_equal(lin['probs'], PROBS)
    assert lin['quantiles'].shape == (5, n)
    np.testing.assert_allclose(lin['quantiles'], np.quantile(f, PROBS, axis=0, method='linear'), rtol=1e-13)
    mean = M.predict_quantiles(Xs, site_sizes=cnt)       # the default scale
    assert mean['scale'] == 'mean'
    np.testing.assert_allclose(mean['quantiles'], np.quantile(pq.stable_sigmoid(f), PROBS, axis=0, method='linear'),
                               rtol=1e-13)
    assert np.all((mean['quantiles'] > 0) & (mean['quantiles'] < 1)) and np.all(np.diff(mean['quantiles'], axis=0) >= 0)
    one = M.predict_quantiles(Xs, probs=0.5, site_sizes=cnt, scale='linear')
    np.testing.assert_array_equal(one['quantiles'], lin['quantiles'][2:3])
    # rows in any order, described by site_ind: the caller's order comes back, to the bit (an order statistic is one of
    # the draws' values and does not depend on its row's place)
    ind = np.repeat(np.arange(4), cnt)
    shuffle = rng.permutation(n)
    for scale, res in (('linear', lin), ('mean', mean)):
        res2 = M.predict_quantiles(Xs[shuffle], site_ind=ind[shuffle], scale=scale)
        np.testing.assert_allclose(res2['quantiles'], res['quantiles'][:, shuffle], rtol=1e-13)
    empty = M.predict_quantiles(Xs[:0], site_sizes=np.zeros(4, dtype=int))
    assert empty['quantiles'].shape == (5, 0)

    # ---- refusals: predict's, and this method's own
    with pytest.raises(ValueError, match='exactly one'):
        M.predict_quantiles(Xs, site_sizes=cnt, site_ind=ind)
    with pytest.raises(ValueError, match='exactly one'):
        M.predict_quantiles(Xs)
    with pytest.raises(ValueError, match='site_sizes'):
        M.predict_quantiles(Xs, site_sizes=cnt + 1)
    with pytest.raises(ValueError, match='site_ind'):
        M.predict_quantiles(Xs, site_ind=np.where(ind == 3, 4, ind))
    with pytest.raises(ValueError, match='X_new'):
        M.predict_quantiles(Xs[:, :1], site_sizes=cnt)
    with pytest.raises(ValueError, match='no `j_ind`'):
        M.predict_quantiles(Xs, site_sizes=cnt, j_ind=np.ones(n, dtype=int))
    with pytest.raises(ValueError, match='scale'):
        M.predict_quantiles(Xs, site_sizes=cnt, scale='logit')
    with pytest.raises(ValueError, match='Bernoulli'):
        M.predict_quantiles(Xs, site_sizes=cnt, scale='response')
    with pytest.raises(ValueError, match='probs'):
        M.predict_quantiles(Xs, site_sizes=cnt, probs=(0.5, 1.5))
    for seed in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError, match='seed'):
            M.predict_quantiles(Xs, site_sizes=cnt, seed=seed)

    def from_cavity(data, stan_params):                  # draws of phi alone, as an injector gives them
        z = np.random.RandomState(stan_params['seed'] % 1000).randn(80, 6)
        return data['mu_phi'] + np.linalg.solve(np.linalg.cholesky(data['Omega_phi']).T, z.T).T
    M._sample_injector = from_cavity
    M.run(1, verbose=False, seed=3)
    with pytest.raises(RuntimeError, match='injected'):
        M.predict_quantiles(Xs, site_sizes=cnt)


def test_master_quantiles_with_several_groups_per_site():
    M = _master('m4b', 7, 3)                             # 7 groups on 3 sites
    M.run(1, verbose=False, seed=3)
    Nk, j_ind = np.diff(M.k_lim), np.asarray(M.A_n['j_ind'])
    f = _f_by_site(M, M.X, Nk, j_ind - 1)
    res = M.predict_quantiles(M.X, site_sizes=Nk, j_ind=j_ind, scale='linear')
    np.testing.assert_allclose(res['quantiles'], np.quantile(f, PROBS, axis=0, method='linear'), rtol=1e-13)
    shuffle = np.random.RandomState(1).permutation(M.X.shape[0])
    ind = np.repeat(np.arange(3), Nk)
    res2 = M.predict_quantiles(M.X[shuffle], site_ind=ind[shuffle], j_ind=j_ind[shuffle])
    np.testing.assert_allclose(res2['quantiles'], np.quantile(pq.stable_sigmoid(f), PROBS, axis=0, method='linear')[:, shuffle],
                               rtol=1e-13)
    with pytest.raises(ValueError, match='`j_ind`'):
        M.predict_quantiles(M.X, site_sizes=Nk)
    bad = j_ind.copy()
    bad[5] = int(M._site_ng[0]) + 1
    with pytest.raises(ValueError, match='row 5: group %d outside' % bad[5]):
        M.predict_quantiles(M.X, site_sizes=Nk, j_ind=bad)


def test_master_quantiles_of_the_replicated_response():
    M = _master('m4a', 4, 2)                             # Gaussian family, two groups per site
    M.run(1, verbose=False, seed=3)
    Nk, j_ind = np.diff(M.k_lim), np.asarray(M.A_n['j_ind'])
    n = M.X.shape[0]
    res = M.predict_quantiles(M.X, site_sizes=Nk, j_ind=j_ind, scale='response', seed=7)
    # the statement, row by row: the replicate of caller's row i under draw s of its site
    mid, gauss, _ = M._site_spec()
    assert gauss
    thetas = [M.engine.get_draws(k, all_params=True) for k in range(M.K)]
    f = _f_by_site(M, M.X, Nk, j_ind - 1)
    sig = np.concatenate([np.repeat(np.exp(thetas[k][:, :1]), Nk[k], axis=1) for k in range(M.K)], axis=1)
    v = f + sig * ppc.replicate_normals(7, np.arange(n), f.shape[0], kind=pq.K_PRED_REP)
    np.testing.assert_allclose(res['quantiles'], np.quantile(v, PROBS, axis=0, method='linear'), rtol=1e-13)
    band = M.predict_quantiles(M.X, site_sizes=Nk, j_ind=j_ind, scale='mean')
    np.testing.assert_allclose(band['quantiles'], np.quantile(f, PROBS, axis=0, method='linear'), rtol=1e-13)
    width = res['quantiles'][-1] - res['quantiles'][0]
    assert np.all(width > band['quantiles'][-1] - band['quantiles'][0])      # the response's interval holds sigma's share
    # a row keeps its replicates wherever it stands in the call
    shuffle = np.random.RandomState(2).permutation(n)
    ind = np.repeat(np.arange(M.K), Nk)
    res2 = M.predict_quantiles(M.X[shuffle], site_ind=ind[shuffle], j_ind=j_ind[shuffle], scale='response', seed=7)
    assert not np.array_equal(res2['quantiles'], res['quantiles'])           # (row i of this call is another row ...)
    v2 = f[:, shuffle] + sig[:, shuffle] * ppc.replicate_normals(7, np.arange(n), f.shape[0], kind=pq.K_PRED_REP)
    np.testing.assert_allclose(res2['quantiles'], np.quantile(v2, PROBS, axis=0, method='linear'), rtol=1e-13)
    # ... and the SAME rows in the same places of the call, described the other way, have the same result
    res3 = M.predict_quantiles(M.X, site_ind=ind, j_ind=j_ind, scale='response', seed=7)
    np.testing.assert_array_equal(res3['quantiles'], res['quantiles'])
    other = M.predict_quantiles(M.X, site_sizes=Nk, j_ind=j_ind, scale='response', seed=8)
    assert np.all(other['quantiles'] != res['quantiles'])
    lin = M.predict_quantiles(M.X, site_sizes=Nk, j_ind=j_ind, scale='linear', seed=8)
    np.testing.assert_array_equal(lin['quantiles'], band['quantiles'])       # f does not see the seed
    Mb = _master('m4b', 4, 2)
    Mb.run(1, verbose=False, seed=3)
    with pytest.raises(ValueError, match='Bernoulli'):
        Mb.predict_quantiles(Mb.X, site_sizes=np.diff(Mb.k_lim), j_ind=np.asarray(Mb.A_n['j_ind']), scale='response')


# ------------------------------------------------------------------ the resolver
def test_intervals_resolve_like_the_queries():
    assert dq.INTERVALS == ('predict_order_stats',)
    assert not set(dq.INTERVALS) & (set(dq.QUERIES) | set(dq.CHECKS))
    assert len(dq.QUERIES) == 8 and dq.CHECKS == ('replicated_checks',)
    host, device = (inspect.signature(getattr(c, 'predict_order_stats')) for c in (dq.HostDraws, HipEngine))
    assert list(host.parameters)[:8] == list(device.parameters)[:8]
    for par in host.parameters.values():
        assert par.name in device.parameters and par.default == device.parameters[par.name].default, par.name
    assert [p for p in device.parameters if p not in host.parameters] == ['k0', 'count', 'theta']

    class Sampling(object):
        def get_draws(self, k, all_params=False):
            return np.zeros((3, 5))

        def num_draws(self):
            return 3

    class WithDevice(Sampling):
        def predict_order_stats(self, *a, **kw):
            return 'device'
    engines = [Sampling()]
    host = dq.HostDraws(lambda: engines[0], (0, False, True), 2, np.ones(1, dtype=np.int64), None, None, None,
                        np.array([0, 0]), 1)
    q = dq.Queries(host)
    assert q.predict_order_stats.__self__ is host
    out, n = q.predict_order_stats(np.ones((2, 2)), np.array([0, 2]), np.array([0, 2]), with_n=True)
    assert out.shape == (2, 2) and n == 3 and np.all(out == 0.0)
    engines[0] = WithDevice()                            # resolved at every call, from the engine at that time
    assert q.predict_order_stats() == 'device'
    with pytest.raises(AttributeError):
        q.predict_quantiles


# ------------------------------------------------------------------ the row collective
class _TwoRanks(object):
    """Rank `rank` of two: allreduce_sum adds what the other rank contributes (given at construction) to the buffer."""
    world = 2

    def __init__(self, rank, other):
        self.rank, self.other = rank, other

    def allreduce_sum(self, buf):
        buf += self.other
        return buf


def test_sum_order_rows_carries_every_value_unchanged():
    n, T, cut = 7, 3, 4
    rng = np.random.RandomState(0)
    full = rng.randn(n, T)
    full[0, 1], full[1, :], full[2, 0], full[2, 2] = np.inf, np.nan, -np.inf, -0.0       # rank 0's block
    full[4, :], full[5, 0], full[6, 1], full[6, 2] = np.nan, -np.inf, np.inf, 0.0        # rank 1's block
    single = type('One', (), {'world': 1})()
    assert dq.sum_order_rows(single, full, 0, n, n) is full
    # what each rank puts into the sum: its own call against a communicator that adds nothing
    sent = []

    class Tap(_TwoRanks):
        def allreduce_sum(self, buf):
            sent.append(buf.copy())
            return buf
    for lo, hi in ((0, cut), (cut, n)):
        dq.sum_order_rows(Tap(0, None), full[lo:hi], lo, hi, n)
    assert len(sent) == 2 and sent[0].shape == (n, 2 * T) and np.all(np.isfinite(sent[0])) and np.all(np.isfinite(sent[1]))
    assert np.all(sent[0][cut:] == 0.0) and np.all(sent[1][:cut] == 0.0)                 # zero-filled outside its rows
    for rank, (lo, hi) in enumerate(((0, cut), (cut, n))):
        got = dq.sum_order_rows(_TwoRanks(rank, sent[1 - rank]), full[lo:hi], lo, hi, n)
        assert got.shape == (n, T)
        nan = np.isnan(full)
        np.testing.assert_array_equal(np.isnan(got), nan)
        np.testing.assert_array_equal(got[~nan].view(np.uint64), full[~nan].view(np.uint64))     # bit for bit
