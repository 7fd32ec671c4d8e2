"""`newgroup` and `Master.predict_new_group` on the CPU: the NumPy Philox stream against the oracle's bit for bit, the
NumPy statement of the new-group predictive against a brute-force extended-precision loop written from the definition
(include/epx.h, epx_predict_new_group), the merge of disjoint pools, known answers in distribution, and
`Master.predict_new_group`'s bookkeeping with the oracle standing in for the device engine, on one rank and on two over
gloo."""

import os
import socket
import sys

import numpy as np
import pytest

from epstan_amd import models, newgroup, site_params
from epstan_amd.method import Master
from epstan_amd.util import distribute_groups
from oracle import nuts_oracle
from oracle.engine_oracle import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
PI = 4 * np.arctan(LD(1))
MEAN, F_MEAN, F_M2, LPD = site_params.PR_MEAN, site_params.PR_F_MEAN, site_params.PR_F_M2, site_params.PR_LPD


def factory(model, X, y, k_lim, **groups):
    return OracleEngine(model, X, y, k_lim, **groups)


# ------------------------------------------------------------------ 1. the stream
def test_numpy_philox_equals_the_oracles_bit_for_bit():
    big = 2 ** 32 - 1
    cases = [(0, 0, 0, 6, 0, 0), (1, 0, 1, 6, 0, 1), (12345, 7, 99, 6, 3, 2), (2 ** 32, 100000, big, 6, 64, big),
             (2 ** 63 + 12345678901, 2 ** 31 - 1, 2 ** 31, 6, 1, 1023), (2 ** 64 - 1, 3, big - 1, 6, 0, big - 1),
             (77, 12, 2 ** 31 - 1, 6, 5, 0), (5, 0, 17, newgroup.K_NEWGROUP, 2, 3)]
    for seed, chain, t, kind, a, b in cases:
        exp = nuts_oracle.rng_probe(seed, chain, t, kind, a, b)
        u1, u2 = newgroup.rng_u2(newgroup.make_key(seed, chain), np.array([t]), kind, a, np.array([b]))
        assert (float(u1[0]), float(u2[0])) == exp[:2], (seed, chain, t, kind, a, b)
        assert 0.0 < u1[0] < 1.0 and 0.0 < u2[0] < 1.0
    # vectorised over t and b at once: the same numbers as one at a time
    t, b = np.array([0, 5, big])[:, None], np.array([0, 1, big])[None, :]
    u1, u2 = newgroup.rng_u2(newgroup.make_key(2 ** 40 + 3, 9), t, 6, 2, b)
    for i in range(3):
        for j in range(3):
            assert (u1[i, j], u2[i, j]) == nuts_oracle.rng_probe(2 ** 40 + 3, 9, int(t[i, 0]), 6, 2, int(b[0, j]))[:2]
    # the normal latents are rng_normal's pair, cosine first
    z = newgroup.latents_host(3, 3, 12345, 7, np.array([99]), 3)
    for r in range(3):
        for p in range(2):
            n0, n1 = nuts_oracle.rng_probe(12345, 7, 99, 6, p, r)[2:]
            np.testing.assert_allclose(z[0, r, 2 * p:2 * p + 2], [n0, n1], rtol=1e-14, atol=1e-15)


# ------------------------------------------------------------------ 2. against a long-double loop
def _brute_latent(mid, seed, label, t, r, e):
    u1, u2 = nuts_oracle.rng_probe(seed, label, t, 6, e >> 1, r)[:2]
    if mid == 4:
        x = LD(u2 if e & 1 else u1) - LD(0.5)
        return -np.sign(x) * np.log1p(-2 * abs(x))
    rad, ang = np.sqrt(-2 * np.log(LD(u1))), 2 * PI * LD(u2)
    return rad * (np.sin(ang) if e & 1 else np.cos(ang))


def _coefficients(mid, D, gauss, th, z):
    """(alpha, beta (D)) of the new group from ONE phi draw and its latents, straight from the Stan programs."""
    b = th.astype(LD)[(1 if gauss else 0):]
    if mid == 0:                                         # phi = [log sigma_a, beta]
        return z[0] * np.exp(b[0]), [b[1 + j] for j in range(D)]
    if mid == 1:                                         # phi = [log sigma_a, log sigma_b]
        return z[0] * np.exp(b[0]), [z[1 + j] * np.exp(b[1]) for j in range(D)]
    if mid == 2:                                         # phi = [log sigma_a, log sigma_b (D)]
        return z[0] * np.exp(b[0]), [z[1 + j] * np.exp(b[1 + j]) for j in range(D)]
    # phi = [mu_a, log sigma_a, mu_b (D), log sigma_b (D)]
    return b[0] + z[0] * np.exp(b[1]), [b[2 + j] + z[1 + j] * np.exp(b[2 + D + j]) for j in range(D)]


def _brute(mid, D, gauss, phi, Xn, gidx, labels, y, seed, t0, R):
    count, S = phi.shape[:2]
    N, n, G = count * S * R, Xn.shape[0], len(labels)
    E = 1 if mid == 0 else 1 + D
    rows, glpd = np.zeros((n, 4), dtype=LD), np.zeros(G, dtype=LD)
    for g in range(G):
        at = np.nonzero(gidx == g)[0]
        f, mu, ll = [np.zeros((N, len(at)), dtype=LD) for _ in range(3)]
        for b in range(count):
            for s in range(S):
                for r in range(R):
                    m, t = (b * S + s) * R + r, t0 + b * S + s
                    z = [_brute_latent(mid, seed, int(labels[g]), t, r, e) for e in range(E)]
                    alpha, beta = _coefficients(mid, D, gauss, phi[b, s], z)
                    for c, i in enumerate(at):
                        f[m, c] = alpha + sum(LD(Xn[i, j]) * beta[j] for j in range(D))
                        if gauss:
                            ls = LD(phi[b, s, 0])
                            mu[m, c] = f[m, c]
                            ll[m, c] = -LD(0.5) * np.log(2 * PI) - ls - LD(0.5) * ((LD(y[i]) - f[m, c]) / np.exp(ls)) ** 2
                        else:
                            mu[m, c] = 1 / (1 + np.exp(-f[m, c]))
                            ll[m, c] = LD(y[i]) * f[m, c] - np.log1p(np.exp(f[m, c]))
        rows[at, 0] = mu.sum(axis=0) / N
        rows[at, 1] = f.sum(axis=0) / N
        rows[at, 2] = ((f - rows[at, 1]) ** 2).sum(axis=0)
        rows[at, 3] = np.log(np.exp(ll).sum(axis=0) / N)
        glpd[g] = np.log(np.exp(ll.sum(axis=1)).sum() / N) if len(at) else 0
    return rows.astype(np.float64), glpd.astype(np.float64)


def _problem(mid, gauss, D=3, S=7, count=3, seed=0):
    rng = np.random.RandomState(10 * mid + gauss + seed)
    d = site_params.layout(mid, D, 1, gauss)[1]
    phi = 0.5 * rng.randn(count, S, d) + 0.3
    gidx = np.array([0, 2, 2, 0, 2, 0, 0, 2, 2, 2, 0])   # 11 rows in 3 groups, group 1 without rows
    labels = np.array([7, 0, 100000])
    n = gidx.shape[0]
    Xn = 1.5 * rng.randn(n, D)
    y = 0.4 + rng.randn(n) if gauss else (rng.rand(n) < 0.5).astype(float)
    return phi, Xn, gidx, labels, y


CASES = [(0, False), (1, False), (3, False), (4, False), (3, True)]
IDS = ['m1b_sg', 'm2b_sg', 'm4b_sg', 'm5b_sg', 'm4a_sg']


@pytest.mark.parametrize('mid,gauss', CASES, ids=IDS)
def test_host_statement_against_a_long_double_loop(mid, gauss):
    D, R, seed, t0 = 3, 2, 2 ** 33 + 5, 2 ** 31 - 4      # the pooled draws straddle 2^31
    phi, Xn, gidx, labels, y = _problem(mid, gauss)
    rows, glpd, N = newgroup.predict_new_group_host(mid, D, gauss, phi, Xn, gidx, labels, y, seed, t0, R)
    assert N == 3 * 7 * 2 and rows.shape == (11, 4) and glpd.shape == (3,)
    erows, eglpd = _brute(mid, D, gauss, phi, Xn, gidx, labels, y, seed, t0, R)
    np.testing.assert_allclose(rows, erows, rtol=1e-12)
    np.testing.assert_allclose(glpd, eglpd, rtol=1e-12)
    assert glpd[1] == 0.0 and np.all(glpd[[0, 2]] < 0)
    # the rows of a group share the member's latents: the joint term is not the sum of the rows'
    for g in (0, 2):
        assert abs(glpd[g] - rows[gidx == g, LPD].sum()) > 1e-3
    none = newgroup.predict_new_group_host(mid, D, gauss, phi, Xn, gidx, labels, None, seed, t0, R)
    assert np.all(np.isnan(none[0][:, LPD])) and np.all(np.isnan(none[1]))
    np.testing.assert_array_equal(none[0][:, :3], rows[:, :3])
    if gauss:
        np.testing.assert_array_equal(rows[:, MEAN], rows[:, F_MEAN])
    # a latent depends on (seed, label, t, r, e) only: other rows and groups may come or go
    keep = gidx == 2
    sub = newgroup.predict_new_group_host(mid, D, gauss, phi, Xn[keep], None, labels[2:], y[keep], seed, t0, R)
    np.testing.assert_allclose(sub[0], rows[keep], rtol=1e-13)
    np.testing.assert_allclose(sub[1], glpd[2:], rtol=1e-13)
    with pytest.raises(ValueError, match='gidx'):
        newgroup.predict_new_group_host(mid, D, gauss, phi, Xn, np.full(11, 3), labels, y, seed, t0, R)
    with pytest.raises(ValueError, match='labels'):
        newgroup.predict_new_group_host(mid, D, gauss, phi, Xn, gidx, [7, -1, 3], y, seed, t0, R)
    with pytest.raises(ValueError, match='R must'):
        newgroup.predict_new_group_host(mid, D, gauss, phi, Xn, gidx, labels, y, seed, t0, 0)
    with pytest.raises(ValueError, match='2\\^32'):
        newgroup.predict_new_group_host(mid, D, gauss, phi, Xn, gidx, labels, y, seed, 2 ** 32 - 20, R)
    empty = newgroup.predict_new_group_host(mid, D, gauss, phi, Xn[:0], None, labels, y[:0], seed, t0, R)
    assert empty[0].shape == (0, 4) and np.all(empty[1] == 0.0) and empty[2] == N


# ------------------------------------------------------------------ 3. merging disjoint pools
@pytest.mark.parametrize('mid,gauss', CASES, ids=IDS)
@pytest.mark.parametrize('cuts', [(0, 1, 5), (0, 4, 5), (0, 2, 3, 5), (0, 1, 2, 3, 4, 5)])
def test_any_split_of_the_pool_by_sites_merges_to_the_whole(mid, gauss, cuts):
    D, S, R, seed, t0 = 3, 6, 3, 11, 40
    phi, Xn, gidx, labels, y = _problem(mid, gauss, S=S, count=5, seed=1)
    whole = newgroup.predict_new_group_host(mid, D, gauss, phi, Xn, gidx, labels, y, seed, t0, R)
    parts = [newgroup.predict_new_group_host(mid, D, gauss, phi[lo:hi], Xn, gidx, labels, y, seed, t0 + lo * S, R)
             for lo, hi in zip(cuts[:-1], cuts[1:])]
    rows, glpd, N = newgroup.merge(parts)
    assert N == whole[2] == 5 * S * R
    np.testing.assert_allclose(rows, whole[0], rtol=1e-12)
    np.testing.assert_allclose(glpd, whole[1], rtol=1e-12)
    assert glpd[1] == 0.0
    bare = newgroup.merge([newgroup.predict_new_group_host(mid, D, gauss, phi[lo:hi], Xn, gidx, labels, None, seed,
                                                           t0 + lo * S, R) for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert np.all(np.isnan(bare[0][:, LPD])) and np.all(np.isnan(bare[1]))
    np.testing.assert_array_equal(bare[0][:, :3], rows[:, :3])


# ------------------------------------------------------------------ 4. known answers in distribution
def test_moments_of_the_linear_predictor_under_a_constant_pool():
    """phi the same in every draw: f = mu_a + x . mu_b + sigma_a eta + sum_j x_j sigma_bj etb_j with independent latents.
    Bounds: five standard errors of the sample mean and of the sample variance, Var(s^2) = (mu_4 - sigma^4) / N."""
    D, count, S, R = 3, 4, 500, 4
    N = count * S * R
    assert N >= 8000
    mu_a, sig_a = 0.7, 0.6
    mu_b, sig_b = np.array([0.3, -0.5, 0.2]), np.array([0.4, 0.9, 0.25])
    Xn = np.array([[1.0, -2.0, 0.5], [0.0, 0.0, 0.0], [0.3, 0.1, -1.2]])
    # m4a_sg: phi = [log sigma | mu_a, log sigma_a, mu_b, log sigma_b]; normal latents, f is normal: mu_4 = 3 sigma^4
    phi = np.tile(np.concatenate(([0.1, mu_a, np.log(sig_a)], mu_b, np.log(sig_b))), (count, S, 1))
    rows, _, n = newgroup.predict_new_group_host(3, D, True, phi, Xn, None, [5], None, 20240, 0, R)
    assert n == N
    var = sig_a ** 2 + (Xn ** 2 * sig_b ** 2).sum(axis=1)
    mean = mu_a + Xn.dot(mu_b)
    assert np.all(np.abs(rows[:, F_MEAN] - mean) <= 5 * np.sqrt(var / N))
    assert np.all(np.abs(rows[:, F_M2] / (N - 1) - var) <= 5 * np.sqrt(2 * var ** 2 / N))
    # m5b_sg at x = 0: f = mu_a + sigma_a Laplace(0, 1): variance 2 sigma_a^2, mu_4 = 24 sigma_a^4
    phi5 = np.tile(np.concatenate(([mu_a, np.log(sig_a)], mu_b, np.log(sig_b))), (count, S, 1))
    r5, _, _ = newgroup.predict_new_group_host(4, D, False, phi5, np.zeros((1, D)), None, [5], None, 20240, 0, R)
    assert abs(r5[0, F_MEAN] - mu_a) <= 5 * np.sqrt(2 * sig_a ** 2 / N)
    assert abs(r5[0, F_M2] / (N - 1) - 2 * sig_a ** 2) <= 5 * np.sqrt((24 - 4) * sig_a ** 4 / N)
    # ... and away from 0 the etb terms add 2 x_j^2 sigma_bj^2
    r5x, _, _ = newgroup.predict_new_group_host(4, D, False, phi5, Xn[:1], None, [5], None, 20240, 0, R)
    v5 = 2 * var[0]
    s4 = sig_a ** 4 + (Xn[0] ** 4 * sig_b ** 4).sum()     # independent terms: mu_4 = sum m_k + 3 ((sum v_k)^2 - sum v_k^2)
    mu4 = 24 * s4 + 3 * (v5 ** 2 - 4 * s4)
    assert abs(r5x[0, F_M2] / (N - 1) - v5) <= 5 * np.sqrt((mu4 - v5 ** 2) / N)


@pytest.mark.parametrize('mid,gauss', [(3, True), (4, False), (1, False)], ids=['m4a_sg', 'm5b_sg', 'm2b_sg'])
def test_scales_of_exp_minus_800_drop_the_latents(mid, gauss):
    D = 3
    rng = np.random.RandomState(3)
    d = site_params.layout(mid, D, 1, gauss)[1]
    o = 1 if gauss else 0
    phi = rng.randn(1, 1, d)
    Xn = rng.randn(4, D)
    if mid >= 3:
        phi[0, 0, o + 1], phi[0, 0, o + 2 + D:] = -800.0, -800.0
        alpha, beta = phi[0, 0, o], phi[0, 0, o + 2:o + 2 + D]
    else:
        phi[0, 0, o:] = -800.0
        alpha, beta = 0.0, np.zeros(D)
    rows, _, N = newgroup.predict_new_group_host(mid, D, gauss, phi, Xn, None, [3], None, 9, 0, 1)
    assert N == 1
    closed = (alpha + np.matmul(beta[None, None, :], Xn.T)).reshape(-1)      # no latent anywhere
    np.testing.assert_array_equal(rows[:, F_MEAN], closed)
    assert np.all(rows[:, F_M2] == 0.0)


# ------------------------------------------------------------------ 5. Master.predict_new_group
def _sg_master(**kw):
    kw.setdefault('_engine_factory', factory)
    mod = models.m4b(4, 2, 15)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    return Master('m4b_sg', data.X, data.y, site_sizes=data.Nj, prior={'Q': Q0, 'r': r0}, chains=4, iter=40, df0=0.4,
                  **kw), data


def _groups_master(**kw):
    kw.setdefault('_engine_factory', factory)
    mod = models.m4b(7, 2, 25)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    Nk, Nj_k, j_ind_k = distribute_groups(7, 3, data.Nj)
    return Master('m4b', data.X, data.y, site_sizes=Nk, A_k={'J': Nj_k}, A_n={'j_ind': j_ind_k + 1},
                  prior={'Q': Q0, 'r': r0}, chains=4, iter=40, df0=0.4, **kw)


def _new_rows(D, n=13, seed=4):
    rng = np.random.RandomState(seed)
    group = rng.permutation(np.array([12] * 5 + [3] * 6 + [70000] * 2))[:n]      # labels in shuffled order
    return rng.randn(n, D), group, (rng.rand(n) < 0.5).astype(int)


def test_master_predict_new_group_rows_groups_seeds_and_refusals():
    M, data = _sg_master()
    Xs, group, ys = _new_rows(2)
    with pytest.raises(RuntimeError, match='at least one iteration'):
        M.predict_new_group(Xs, group)
    M.run(1, verbose=False, seed=2)
    res = M.predict_new_group(Xs, group, y_new=ys, R=2, seed=31)
    assert set(res) == {'mean', 'f_mean', 'f_var', 'lpd', 'groups', 'group_lpd', 'n'}
    N = 4 * 80 * 2
    assert res['n'] == N and list(res['groups']) == [3, 12, 70000]
    phi = np.stack([np.ascontiguousarray(M.engine.get_draws(k)) for k in range(4)])
    gidx = np.searchsorted([3, 12, 70000], group)
    rows, glpd, _ = newgroup.predict_new_group_host(3, 2, False, phi, Xs, gidx, [3, 12, 70000], ys.astype(float), 31, 0, 2)
    np.testing.assert_allclose(res['mean'], rows[:, MEAN], rtol=1e-12)
    np.testing.assert_allclose(res['f_mean'], rows[:, F_MEAN], rtol=1e-12)
    np.testing.assert_allclose(res['f_var'], rows[:, F_M2] / (N - 1), rtol=1e-12)
    np.testing.assert_allclose(res['lpd'], rows[:, LPD], rtol=1e-12)
    np.testing.assert_allclose(res['group_lpd'], glpd, rtol=1e-12)
    assert np.all((res['mean'] > 0) & (res['mean'] < 1)) and np.all(res['f_var'] > 0) and np.all(res['lpd'] < 0)
    for g in res['groups']:
        at = group == g
        assert abs(res['lpd'][at].sum() - res['group_lpd'][list(res['groups']).index(g)]) > 1e-6
    # rows in any order: the caller's order comes back
    shuffle = np.random.RandomState(1).permutation(len(group))
    res2 = M.predict_new_group(Xs[shuffle], group[shuffle], y_new=ys[shuffle], R=2, seed=31)
    for key in ('mean', 'f_mean', 'f_var', 'lpd'):
        np.testing.assert_allclose(res2[key], res[key][shuffle], rtol=1e-12)
    np.testing.assert_allclose(res2['group_lpd'], res['group_lpd'], rtol=1e-12)
    # other rows and groups dropped from the call: a row's record stays
    keep = np.nonzero(group != 12)[0][1:]
    res3 = M.predict_new_group(Xs[keep], group[keep], y_new=ys[keep], R=2, seed=31)
    assert list(res3['groups']) == [3, 70000]
    for key in ('mean', 'f_mean', 'f_var', 'lpd'):
        np.testing.assert_allclose(res3[key], res[key][keep], rtol=1e-12)
    # the same seed reproduces, another seed differs; no responses: no densities
    again = M.predict_new_group(Xs, group, y_new=ys, R=2, seed=31)
    for key in ('mean', 'f_mean', 'f_var', 'lpd', 'group_lpd'):
        np.testing.assert_array_equal(again[key], res[key])
    other = M.predict_new_group(Xs, group, y_new=ys, R=2, seed=32)
    assert np.all(other['f_mean'] != res['f_mean']) and np.all(other['group_lpd'] != res['group_lpd'])
    bare = M.predict_new_group(Xs, group, R=2, seed=31)
    assert bare['lpd'] is None and bare['group_lpd'] is None
    np.testing.assert_array_equal(bare['mean'], res['mean'])
    one = M.predict_new_group(Xs, y_new=ys)                               # one group, label 0, R = 1, seed 0
    assert list(one['groups']) == [0] and one['n'] == 320 and one['group_lpd'].shape == (1,)
    empty = M.predict_new_group(Xs[:0], group[:0])
    assert empty['mean'].shape == (0,) and empty['groups'].shape == (0,) and empty['n'] == 320

    # ---- refusals
    with pytest.raises(ValueError, match='X_new'):
        M.predict_new_group(Xs[:, :1], group)
    with pytest.raises(ValueError, match='`group`'):
        M.predict_new_group(Xs, group[:-1])
    with pytest.raises(ValueError, match='`group`'):
        M.predict_new_group(Xs, group.astype(float))
    with pytest.raises(ValueError, match='row 4: label -1'):
        M.predict_new_group(Xs, np.where(np.arange(13) == 4, -1, group))
    with pytest.raises(ValueError, match='row 2: label'):
        M.predict_new_group(Xs, np.where(np.arange(13) == 2, 2 ** 31, group.astype(np.int64)))
    with pytest.raises(ValueError, match='y_new'):
        M.predict_new_group(Xs, group, y_new=ys[:-1])
    with pytest.raises(ValueError, match='row 6.*0 or 1'):
        M.predict_new_group(Xs, group, y_new=np.where(np.arange(13) == 6, 2, ys))
    for R in (0, 1025, 1.5, True):
        with pytest.raises(ValueError, match='`R`'):
            M.predict_new_group(Xs, group, R=R)
    for seed in (-1, 2 ** 64, 0.5):
        with pytest.raises(ValueError, match='`seed`'):
            M.predict_new_group(Xs, group, seed=seed)

    def from_cavity(data, stan_params):                  # draws of phi alone, as an injector gives them
        z = np.random.RandomState(stan_params['seed'] % 1000).randn(80, 6)
        return data['mu_phi'] + np.linalg.solve(np.linalg.cholesky(data['Omega_phi']).T, z.T).T
    M._sample_injector = from_cavity
    M.run(1, verbose=False, seed=3)
    with pytest.raises(RuntimeError, match='injected'):
        M.predict_new_group(Xs, group)


# ------------------------------------------------------------------ two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _predict(M):
    Xs, group, ys = _new_rows(2)
    return M.predict_new_group(Xs, group, y_new=ys, R=3, seed=2 ** 40 + 1)


KEYS = ('mean', 'f_mean', 'f_var', 'lpd', 'group_lpd')


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
    import test_newgroup_host as me
    tdist.init_process_group('gloo', rank=rank, world_size=world)
    fac = lambda m, X, y, kl, **g: OracleEngine(m, X, y, kl, nthreads=2, **g)
    M = me._groups_master(comm=dist.TorchComm(), _engine_factory=fac)
    M.run(1, verbose=False, seed=3)
    res = me._predict(M)
    assert res['n'] == 3 * 80 * 3
    np.savez(os.path.join(outdir, 'r%d.npz' % rank), **dict((k, res[k]) for k in KEYS))
    bare = M.predict_new_group(me._new_rows(2)[0], me._new_rows(2)[1], R=3, seed=2 ** 40 + 1)
    assert bare['lpd'] is None and np.array_equal(bare['f_mean'], res['f_mean'])
    tdist.barrier()
    tdist.destroy_process_group()


def test_two_ranks_return_the_one_rank_result(tmp_path):
    """3 sites sharded 1 + 2 (a multi-group context: only phi of a record is read): every rank runs all rows against its
    own sites' draws at its own t0, and the merge in rank order returns what one rank returns."""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    M = _groups_master(_engine_factory=lambda m, X, y, kl, **g: OracleEngine(m, X, y, kl, nthreads=2, **g))
    M.run(1, verbose=False, seed=3)
    res = _predict(M)
    assert res['n'] == 3 * 80 * 3 and np.all(np.isfinite(res['lpd'])) and np.all(np.isfinite(res['group_lpd']))
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), 'r%d.npz' % r))
        for key in KEYS:
            np.testing.assert_allclose(z[key], res[key], rtol=1e-12)
