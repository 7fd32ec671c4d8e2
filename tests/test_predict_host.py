"""`site_params.predict_host` and `Master.predict` on the CPU: the NumPy statement of the posterior predictive against a
brute-force extended-precision loop over draws and rows, and `Master.predict`'s bookkeeping (rows by site in either
description, groups within sites, the caller's row order, every refusal) with the oracle standing in for the device
engine, on one rank and on two over gloo."""

import os
import socket
import sys

import numpy as np
import pytest

from epstan_amd import models, site_params
from epstan_amd.method import Master
from epstan_amd.util import distribute_groups
from oracle.engine_oracle import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def factory(model, X, y, k_lim, **groups):
    return OracleEngine(model, X, y, k_lim, **groups)


def _coefficients(mid, D, ng, gauss, th, g):
    """(alpha, beta (D)) of group g from ONE draw, straight from the Stan programs' `transformed parameters`."""
    th = th.astype(LD)
    o = 1 if gauss else 0
    if mid == 0:                                         # phi = [log sigma_a, beta]
        d = o + 1 + D
        return th[d + g] * np.exp(th[o]), th[o + 1:o + 1 + D]
    assert mid == 3                                      # phi = [mu_a, log sigma_a, mu_b (D), log sigma_b (D)]
    d = o + 2 + 2 * D
    etb = th[d + ng + g * D:d + ng + (g + 1) * D]
    return th[o] + th[d + g] * np.exp(th[o + 1]), th[o + 2:o + 2 + D] + etb * np.exp(th[o + 2 + D:o + 2 + 2 * D])


def _brute(mid, D, ng, gauss, theta, Xn, group, y):
    S, n = theta.shape[0], Xn.shape[0]
    out = np.zeros((n, 4), dtype=LD)
    for i in range(n):
        f, mu, ll = np.zeros(S, dtype=LD), np.zeros(S, dtype=LD), np.zeros(S, dtype=LD)
        for s in range(S):
            alpha, beta = _coefficients(mid, D, ng, gauss, theta[s], int(group[i]))
            f[s] = alpha + sum(LD(Xn[i, j]) * beta[j] for j in range(D))
            if gauss:
                ls = LD(theta[s, 0])
                mu[s] = f[s]
                ll[s] = -LD(0.5) * np.log(2 * LD(np.pi)) - ls - LD(0.5) * ((LD(y[i]) - f[s]) / np.exp(ls)) ** 2
            else:
                mu[s] = 1 / (1 + np.exp(-f[s]))
                ll[s] = LD(y[i]) * f[s] - np.log1p(np.exp(f[s]))
        out[i, 0] = mu.sum() / S
        out[i, 1] = f.sum() / S
        out[i, 2] = ((f - out[i, 1]) ** 2).sum()
        out[i, 3] = np.log(np.exp(ll).sum() / S)
    return out.astype(np.float64)


@pytest.mark.parametrize('mid,gauss,ng', [(0, False, 1), (3, False, 1), (3, True, 1), (3, False, 3), (0, False, 2)],
                         ids=['m1b_sg', 'm4b_sg', 'm4a_sg', 'm4b', 'm1b'])
def test_predict_host_against_a_long_double_loop(mid, gauss, ng):
    D, S, n = 3, 23, 11
    rng = np.random.RandomState(10 * mid + ng)
    P = site_params.layout(mid, D, ng, gauss)[1] + ng * (1 + (D if mid else 0))
    theta = 0.5 * rng.randn(S, P) + 0.3
    Xn = 1.5 * rng.randn(n, D)
    group = rng.randint(0, ng, n)
    y = 0.4 + rng.randn(n) if gauss else (rng.rand(n) < 0.5).astype(float)
    got = site_params.predict_host(mid, D, ng, gauss, theta, Xn, group, y)
    assert got.shape == (n, 4) and site_params.PR_COUNT == 4
    np.testing.assert_allclose(got, _brute(mid, D, ng, gauss, theta, Xn, group, y), rtol=1e-12)
    none = site_params.predict_host(mid, D, ng, gauss, theta, Xn, group if ng > 1 else None)
    assert np.all(np.isnan(none[:, site_params.PR_LPD]))
    np.testing.assert_array_equal(none[:, :3], got[:, :3])
    if gauss:
        np.testing.assert_array_equal(got[:, site_params.PR_MEAN], got[:, site_params.PR_F_MEAN])
    with pytest.raises(ValueError, match='group'):
        site_params.predict_host(mid, D, ng, gauss, theta, Xn, np.full(n, ng))
    assert site_params.predict_host(mid, D, ng, gauss, theta, Xn[:0], None).shape == (0, 4)


def test_predict_host_log_mean_exp_survives_saturation():
    """f = -750 in every draw and y = 1: every exp(ll) underflows, the log predictive density is -750 all the same."""
    D, S = 2, 5
    theta = np.zeros((S, 1 + D + 1))                     # m1b_sg: [log sigma_a = 0, beta = 0 | eta]
    theta[:, -1] = -750.0
    out = site_params.predict_host(0, D, 1, False, theta, np.ones((2, D)), None, np.array([1.0, 0.0]))
    assert out[0, site_params.PR_MEAN] == 0.0 and out[0, site_params.PR_F_M2] == 0.0
    np.testing.assert_allclose(out[:, site_params.PR_LPD], [-750.0, 0.0], rtol=1e-12, atol=1e-300)


# ------------------------------------------------------------------ Master.predict
def _sg_master(**kw):
    mod = models.m4b(4, 2, 15)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    return Master('m4b_sg', data.X, data.y, site_sizes=data.Nj, prior={'Q': Q0, 'r': r0}, chains=4, iter=40, df0=0.4,
                  _engine_factory=factory, **kw), data


def _groups_master(**kw):
    kw.setdefault('_engine_factory', factory)
    mod = models.m4b(7, 2, 25)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    Nk, Nj_k, j_ind_k = distribute_groups(7, 3, data.Nj)
    M = Master('m4b', data.X, data.y, site_sizes=Nk, A_k={'J': Nj_k}, A_n={'j_ind': j_ind_k + 1},
               prior={'Q': Q0, 'r': r0}, chains=4, iter=40, df0=0.4, **kw)
    return M, data, Nk, j_ind_k + 1


def _expected(M, Xs, cnt, group, ys):
    """predict_host on the engine's downloaded draws, site by site; rows ordered by site."""
    mid, gauss, _ = M._site_spec()
    lim = np.concatenate(([0], np.cumsum(cnt)))
    return np.concatenate([site_params.predict_host(
        mid, M.D, int(M._site_ng[k]), gauss, M.engine.get_draws(k, all_params=True), Xs[lim[k]:lim[k + 1]],
        None if group is None else group[lim[k]:lim[k + 1]], None if ys is None else ys[lim[k]:lim[k + 1]])
        for k in range(M.K)])


def test_master_predict_by_site_sizes_and_by_shuffled_site_ind():
    M, data = _sg_master()
    with pytest.raises(RuntimeError, match='at least one iteration'):
        M.predict(data.X, site_sizes=data.Nj)
    M.run(1, verbose=False, seed=2)
    rng = np.random.RandomState(4)
    cnt = np.array([5, 0, 7, 3])                         # a site without new rows
    n = int(cnt.sum())
    Xs, ys = rng.randn(n, 2), (rng.rand(n) < 0.5).astype(int)
    res = M.predict(Xs, site_sizes=cnt, y_new=ys)
    assert set(res) == {'mean', 'f_mean', 'f_var', 'lpd', 'n'} and res['n'] == 80
    exp = _expected(M, Xs, cnt, None, ys.astype(float))
    np.testing.assert_allclose(res['mean'], exp[:, 0], rtol=1e-12)
    np.testing.assert_allclose(res['f_mean'], exp[:, 1], rtol=1e-12)
    np.testing.assert_allclose(res['f_var'], exp[:, 2] / 79, rtol=1e-12)
    np.testing.assert_allclose(res['lpd'], exp[:, 3], rtol=1e-12)
    assert np.all((res['mean'] > 0) & (res['mean'] < 1)) and np.all(res['f_var'] > 0) and np.all(res['lpd'] < 0)
    ind = np.repeat(np.arange(4), cnt)
    shuffle = rng.permutation(n)
    res2 = M.predict(Xs[shuffle], site_ind=ind[shuffle], y_new=ys[shuffle])
    for key in ('mean', 'f_mean', 'f_var', 'lpd'):       # the caller's row order: equal after un-shuffling (a row's
        np.testing.assert_allclose(res2[key], res[key][shuffle], rtol=1e-13)     # place may change BLAS's last bit)
    res3 = M.predict(Xs, site_sizes=cnt)
    assert res3['lpd'] is None
    np.testing.assert_array_equal(res3['mean'], res['mean'])
    empty = M.predict(Xs[:0], site_sizes=np.zeros(4, dtype=int))
    assert empty['mean'].shape == (0,) and empty['lpd'] is None

    # ---- refusals
    with pytest.raises(ValueError, match='exactly one'):
        M.predict(Xs, site_sizes=cnt, site_ind=ind)
    with pytest.raises(ValueError, match='exactly one'):
        M.predict(Xs)
    with pytest.raises(ValueError, match='site_sizes'):
        M.predict(Xs, site_sizes=cnt + 1)
    with pytest.raises(ValueError, match='site_sizes'):
        M.predict(Xs, site_sizes=np.array([n + 1, -1, 0, 0]))
    with pytest.raises(ValueError, match='site_ind'):
        M.predict(Xs, site_ind=np.where(ind == 3, 4, ind))
    with pytest.raises(ValueError, match='X_new'):
        M.predict(Xs[:, :1], site_sizes=cnt)
    with pytest.raises(ValueError, match='no `j_ind`'):
        M.predict(Xs, site_sizes=cnt, j_ind=np.ones(n, dtype=int))
    with pytest.raises(ValueError, match='y_new'):
        M.predict(Xs, site_sizes=cnt, y_new=ys[:-1])
    with pytest.raises(ValueError, match='row 6.*0 or 1'):
        M.predict(Xs, site_sizes=cnt, y_new=np.where(np.arange(n) == 6, 2, ys))

    def from_cavity(data, stan_params):                  # draws of phi alone, as an injector gives them
        z = np.random.RandomState(stan_params['seed'] % 1000).randn(80, 6)
        return data['mu_phi'] + np.linalg.solve(np.linalg.cholesky(data['Omega_phi']).T, z.T).T
    M._sample_injector = from_cavity
    M.run(1, verbose=False, seed=3)
    with pytest.raises(RuntimeError, match='injected'):
        M.predict(Xs, site_sizes=cnt)


def test_master_predict_with_several_groups_per_site():
    M, data, Nk, j_ind = _groups_master()                # 7 groups on 3 sites
    M.run(1, verbose=False, seed=3)
    ys = data.y.astype(float)
    res = M.predict(data.X, site_sizes=Nk, j_ind=j_ind, y_new=data.y)
    exp = _expected(M, data.X, Nk, j_ind - 1, ys)
    np.testing.assert_allclose(res['mean'], exp[:, 0], rtol=1e-12)
    np.testing.assert_allclose(res['f_var'], exp[:, 2] / (res['n'] - 1), rtol=1e-12)
    np.testing.assert_allclose(res['lpd'], exp[:, 3], rtol=1e-12)
    # the groups of a site's new rows in any order, rows in any order
    rng = np.random.RandomState(1)
    shuffle = rng.permutation(data.X.shape[0])
    ind = np.repeat(np.arange(3), Nk)
    res2 = M.predict(data.X[shuffle], site_ind=ind[shuffle], j_ind=j_ind[shuffle], y_new=data.y[shuffle])
    for key in ('mean', 'f_mean', 'f_var', 'lpd'):
        np.testing.assert_allclose(res2[key], res[key][shuffle], rtol=1e-13)
    with pytest.raises(ValueError, match='`j_ind`'):
        M.predict(data.X, site_sizes=Nk)
    bad = j_ind.copy()
    bad[5] = int(M._site_ng[0]) + 1
    with pytest.raises(ValueError, match='row 5: group %d outside' % bad[5]):
        M.predict(data.X, site_sizes=Nk, j_ind=bad)
    bad[5] = 0
    with pytest.raises(ValueError, match='row 5'):
        M.predict(data.X, site_sizes=Nk, j_ind=bad)


# ------------------------------------------------------------------ two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _predict_shuffled(M, data, Nk, j_ind):
    shuffle = np.random.RandomState(1).permutation(data.X.shape[0])
    ind = np.repeat(np.arange(3), Nk)
    return M.predict(data.X[shuffle], site_ind=ind[shuffle], j_ind=j_ind[shuffle], y_new=data.y[shuffle])


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
    import test_predict_host as me
    tdist.init_process_group('gloo', rank=rank, world_size=world)
    fac = lambda m, X, y, kl, **g: OracleEngine(m, X, y, kl, nthreads=2, **g)
    M, data, Nk, j_ind = me._groups_master(comm=dist.TorchComm(), _engine_factory=fac)
    M.run(1, verbose=False, seed=3)
    res = me._predict_shuffled(M, data, Nk, j_ind)
    np.savez(os.path.join(outdir, 'r%d.npz' % rank), **dict((k, res[k]) for k in ('mean', 'f_mean', 'f_var', 'lpd')))
    tdist.barrier()
    tdist.destroy_process_group()


def test_two_ranks_predict_equals_one_rank(tmp_path):
    """7 groups on 3 sites, sharded 1 + 2: every rank computes the rows of its own sites, one all-reduce completes the
    array, and both ranks return what one rank returns (the first iteration samples the same draws either way)."""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    M, data, Nk, j_ind = _groups_master(
        _engine_factory=lambda m, X, y, kl, **g: OracleEngine(m, X, y, kl, nthreads=2, **g))
    M.run(1, verbose=False, seed=3)
    res = _predict_shuffled(M, data, Nk, j_ind)
    assert np.all(np.isfinite(res['lpd'])) and np.all(res['f_var'] > 0)
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), 'r%d.npz' % r))
        for key in ('mean', 'f_mean', 'f_var', 'lpd'):
            np.testing.assert_allclose(z[key], res[key], rtol=1e-12)
