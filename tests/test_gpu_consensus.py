"""epx_pooled_moments (csrc/pooled_moments.hip) and the consensus run on the device
(/root/reference/experiment/fit.py:537-675; the pooling of fit.py:639-646).

The kernel is checked on injected draws against np.longdouble sums of the same float64 inputs, within the rounding
bound of ANY summation order (derived, not tuned):
    |sum_i - exact|      <= 2 n u sum_s |x_si - c_i|
    |scatter_ij - exact| <= 2 (n + 4) u sum_s |x_si - c_i||x_sj - c_j|,      u = 2^-53
(n - 1 additions and one product per term, u each; the factor 2 covers the rounding of the centring and the second-order
terms).  The shapes are the smallest that reach every edge of the tiling: one partial tile (d = 2), an edge tile
(d = 34), an odd tile count (d = 66), many tiles with fewer draws than dimensions (d = 258), more than one slab of
draws (n > 128), draws that do not fill a group of four."""

import os
import sys
import threading

import numpy as np
import pytest

from epstan_amd import _lib, dist, fit, models
from epstan_amd.engine import DQI, HipEngine
from epstan_amd.method import Master
from epstan_amd.seeds import MAX_UINT
from test_consensus_host import pooled_bounds
from test_gpu_multirank import _ThreadRank, _ThreadWorld

pytestmark = pytest.mark.gpu
U = 2.0**-53


def _engine(model, D, K, rows=3, g_cnt=None):
    rng = np.random.RandomState(5)
    if g_cnt is None:
        k_lim = np.arange(K + 1) * rows
        kw = {}
    else:
        g_cnt = np.asarray(g_cnt)
        g_lim = np.arange(int(g_cnt.sum()) + 1) * rows
        k_lim = g_lim[np.concatenate(([0], np.cumsum(g_cnt)))]
        kw = dict(g_cnt=g_cnt, g_lim=g_lim)
    N = int(k_lim[-1])
    return HipEngine(model, rng.randn(N, D), (rng.rand(N) < 0.5).astype(np.int32), k_lim, **kw)


def _draws(eng, count, S, seed):
    rng = np.random.RandomState(seed)
    return 0.7 + rng.randn(count, S, eng.P) * (0.5 + rng.rand(eng.P))


def _check(eng, theta, center, k0=0, want_scatter=True):
    """One call on injected draws against the longdouble sums; returns the call's results."""
    count, S, _ = theta.shape
    d = eng.d
    n, s, sc = eng.pooled_moments(center=center, k0=k0, count=count, theta=theta, want_scatter=want_scatter)
    assert n == count * S
    a = theta.reshape(-1, eng.P)[:, :d].astype(np.longdouble)
    if center is not None:
        a = a - np.asarray(center, dtype=np.longdouble)
    absa = np.abs(a)
    err_s = np.abs(s - a.sum(axis=0))
    tol_s = 2 * n * U * absa.sum(axis=0)
    print('d %d n %d: sum err / bound max %.3g' % (d, n, float((err_s / tol_s).max())))
    assert np.all(err_s <= tol_s)
    if not want_scatter:
        assert sc is None
        return n, s, sc
    err = np.abs(sc - a.T.dot(a))
    tol = 2 * (n + 4) * U * absa.T.dot(absa)
    print('d %d n %d: scatter err / bound max %.3g' % (d, n, float((err / tol).max())))
    assert np.all(err <= tol)
    np.testing.assert_array_equal(sc, sc.T)                                 # symmetry is exact
    n2, s2, sc2 = eng.pooled_moments(center=center, k0=k0, count=count, theta=theta)
    assert n2 == n and s2.tobytes() == s.tobytes() and sc2.tobytes() == sc.tobytes()       # the same bits on every call
    return n, s, sc


@pytest.mark.parametrize('model,D,d,K,S,k0,count', [
    ('m2b_sg', 3, 2, 1, 7, 0, 1),           # a single partial tile, one site, draws no multiple of 4
    ('m4b_sg', 16, 34, 5, 61, 0, 5),        # three tiles per side, the last an edge tile; 305 draws: three slabs
    ('m4b_sg', 16, 34, 5, 61, 1, 3),        # a sub-range behind site 0
    ('m4b_sg', 32, 66, 5, 30, 0, 5),        # five tiles per side (odd), two slabs
    ('m4b_sg', 128, 258, 2, 8, 0, 2),       # 17 tiles per side, fewer draws than dimensions
])
def test_pooled_moments_of_injected_draws(model, D, d, K, S, k0, count):
    eng = _engine(model, D, K)
    assert eng.d == d
    theta = _draws(eng, count, S, 11 + d + k0)
    center = theta.reshape(-1, eng.P)[:, :d].mean(axis=0) + 1e-3
    _check(eng, theta, None, k0)                                            # center = NULL
    _check(eng, theta, center, k0)
    n, s0, none = _check(eng, theta, center, k0, want_scatter=False)        # the sums alone, scatter = NULL
    assert s0.tobytes() == eng.pooled_moments(center=center, k0=k0, count=count, theta=theta, want_scatter=False)[1].tobytes()
    with pytest.raises(ValueError):
        eng.pooled_moments(theta=theta[:, :, :-1], k0=k0, count=count)
    with pytest.raises(_lib.EpxError):
        eng.pooled_moments(theta=theta, k0=K - count + 1, count=count)      # a range behind the last site
    eng.close()


def test_pooled_moments_never_read_behind_a_sites_own_coordinates():
    """Sites with 1, 3 and 2 groups: the record stride is the largest site's; what lies behind a smaller site's own
    coordinates (1e300 here) takes no part, and phi -- the first d coordinates -- is all that is pooled."""
    eng = _engine('m4b', 2, 3, g_cnt=[1, 3, 2])
    assert eng.d == 6 and eng.P == 6 + 3 * 3 and list(eng.site_P) == [9, 15, 12]
    theta = _draws(eng, 3, 45, 3)
    for k in range(3):
        theta[k, :, int(eng.site_P[k]):] = 1e300
    for center in (None, np.full(6, 0.7)):
        n, s, sc = _check(eng, theta, center)
        assert np.all(np.isfinite(s)) and np.all(np.isfinite(sc)) and np.abs(sc).max() < 1e6
    eng.close()


def _m1b_master(**kw):
    mod = models.m1b(4, 3, 15)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    return Master('m1b_sg', data.X, data.y, site_sizes=data.Nj, prior={'Q': Q0, 'r': r0}, chains=4, iter=40, df0=0.5, **kw)


def test_pooled_moments_leave_the_site_update_alone_and_refuse_stale_draws():
    M = _m1b_master()
    eng = M.engine
    with pytest.raises(_lib.EpxError, match='no draws yet'):
        eng.pooled_moments()
    assert M.run(1, verbose=False, seed=1)[0] == 0
    dQ, dr = eng.get_sites(DQI)
    tilted = [eng.get_tilted(k) for k in range(4)]
    n, s, sc = eng.pooled_moments(center=np.full(4, 0.1))
    assert n == 4 * 4 * 20
    dQ2, dr2 = eng.get_sites(DQI)
    np.testing.assert_array_equal(dQ, dQ2)
    np.testing.assert_array_equal(dr, dr2)
    for k in range(4):
        for a, b in zip(tilted[k], eng.get_tilted(k)):
            np.testing.assert_array_equal(a, b)
    # a sampling call over sites 1, 2 only: the draws of sites 0 and 3 are stale
    opts = eng.sampler_opts(chains=4, iter=40)
    eng.sample_batch(np.array([5, 6]), opts, k0=1, count=2)
    with pytest.raises(_lib.EpxError, match='the last sampling call left draws of sites'):
        eng.pooled_moments()
    with pytest.raises(_lib.EpxError):
        eng.pooled_moments(k0=2, count=2)
    n, s, sc = eng.pooled_moments(k0=1, count=2)
    x = np.concatenate([eng.get_draws(1), eng.get_draws(2)]).astype(np.longdouble)
    assert n == x.shape[0] == 160
    assert np.all(np.abs(s - x.sum(axis=0)) <= 2 * n * U * np.abs(x).sum(axis=0))
    assert np.all(np.abs(sc - x.T.dot(x)) <= 2 * (n + 4) * U * np.abs(x).T.dot(np.abs(x)))


# ------------------------------------------------------------------ the consensus run on the device
class RecordingEngine(HipEngine):
    """Keeps the pooled phi draws of every sampling call, as the device hands them out."""
    pooled = []

    def sample_batch(self, seeds, opts, k0=0, count=None):
        out = HipEngine.sample_batch(self, seeds, opts, k0, count)
        type(self).pooled.append(np.concatenate([self.get_draws(k) for k in range(self.K)], axis=0))
        return out


def _recording(model, X, y, k_lim, **groups):
    return RecordingEngine(model, X, y, k_lim, **groups)


def _run(model_name, conf, iters, **kw):
    RecordingEngine.pooled = []
    res = fit.main(model_name, conf, verbose=False, iters=iters, _engine_factory=_recording, **kw)
    return res, list(RecordingEngine.pooled)


def _check_run(res, pooled, conf, iters, d):
    assert res['m_s_cons'].shape == (len(iters), d) and res['S_s_cons'].shape == (len(iters), d, d)
    for i, it in enumerate(iters):
        x = pooled[i]
        assert x.shape == (conf.K * conf.chains * (it - it // 2), d)
        m, S, tol_m, tol_S = pooled_bounds(x)
        print('iter %d: mean err / bound %.3g, cov err / bound %.3g' % (it, float((np.abs(res['m_s_cons'][i] - m) / tol_m).max()),
                                                                       float((np.abs(res['S_s_cons'][i] - S) / tol_S).max())))
        assert np.all(np.abs(res['m_s_cons'][i] - m) <= tol_m)
        assert np.all(np.abs(res['S_s_cons'][i] - S) <= tol_S)
        np.testing.assert_array_equal(res['S_s_cons'][i], res['S_s_cons'][i].T)
    for key in ('time_s_cons', 'mstepsize_s_cons', 'mrhat_s_cons'):
        assert res[key].shape == (len(iters),) and np.all(np.isfinite(res[key])) and np.all(res[key] > 0)


@pytest.fixture(scope='module')
def m1b_device_run():
    conf = fit.configurations(J=4, D=3, K=4, npg=15, run_consensus=True, save_res=False)
    res, pooled = _run('m1b', conf, [40, 60])
    return conf, res, pooled


def test_consensus_run_pools_the_devices_own_draws(m1b_device_run):
    conf, res, pooled = m1b_device_run
    _check_run(res, pooled, conf, [40, 60], 4)
    again, pooled2 = _run('m1b', conf, [40, 60])
    for key in ('m_s_cons', 'S_s_cons', 'mstepsize_s_cons', 'mrhat_s_cons'):
        assert again[key].tobytes() == res[key].tobytes()                   # reproducible bit for bit
    seeds = np.random.RandomState(seed=conf.seed_cons).randint(0, MAX_UINT, size=4)
    assert len(set(seeds.tolist())) == 4 and not np.array_equal(pooled[0][:80], pooled[0][80:160])


def test_consensus_run_with_several_groups_per_site():
    conf = fit.configurations(J=6, K=3, D=2, npg=12, run_consensus=True, save_res=False)
    res, pooled = _run('m4b', conf, [40])
    _check_run(res, pooled, conf, [40], 6)


def test_two_ranks_on_one_device_pool_the_draws_of_all_sites(m1b_device_run):
    """Sites sharded 2 + 2 over two ranks -- threads of this process, both on device 0, the library's collectives over a
    host transport: the all-reduced sums give the single-rank moments up to the summation order."""
    conf, res, pooled = m1b_device_run
    _lib.load()
    tw = _ThreadWorld(2, timeout=300.0)
    out, errors = {}, []

    def run(rank):
        try:
            out[rank] = fit.main('m1b', conf, verbose=False, iters=[40, 60], comm=dist.HostComm(_ThreadRank(tw, rank)), device=0)
        except BaseException as ex:
            errors.append(ex)
            tw.barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    for i in range(2):
        _, _, tol_m, tol_S = pooled_bounds(pooled[i])
        for r in range(2):
            assert np.all(np.abs(out[r]['m_s_cons'][i] - res['m_s_cons'][i]) <= tol_m)
            assert np.all(np.abs(out[r]['S_s_cons'][i] - res['S_s_cons'][i]) <= tol_S)
    for key in ('m_s_cons', 'S_s_cons', 'mstepsize_s_cons', 'mrhat_s_cons'):
        assert out[0][key].tobytes() == out[1][key].tobytes()
    assert out[0]['mrhat_s_cons'].tolist() == res['mrhat_s_cons'].tolist()
    np.testing.assert_allclose(out[0]['mstepsize_s_cons'], res['mstepsize_s_cons'], rtol=1e-14)
