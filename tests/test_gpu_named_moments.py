"""k_named_moments / epx_named_moments / Master.mix_pred on the device: per-site moments of the named parameters of the
site models from draws in device memory, against site_params.named_moments_host (NumPy, centred).  Need a real MI355X.

Tolerances: both orders of a centred sum over S <= 400 draws differ by < S 2^-53 ~ 5e-14 relative, the device exp from
libm by ~2e-16: means at rtol 1e-9 + 1e-12 max|x|, centred sums of squares at rtol 1e-9."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from epstan_amd import _lib, fit, models, site_params        # noqa: E402
from epstan_amd.engine import HipEngine, MODEL_IDS, is_gauss  # noqa: E402
from epstan_amd.mix_pred import combine_moments              # noqa: E402
from test_gpu_parity import _site_problem, _engine_with_cavity, _group_problem   # noqa: E402

RTOL = 1e-9


def _spec(model):
    return MODEL_IDS[model] % 5, is_gauss(model), model.endswith('_sg')


def _raw(eng, names, theta=None, k0=0, count=None):
    """The C entry point itself: (n, mean (count, L), m2 (count, L)), rows as the library lays them out."""
    count = eng.K - k0 if count is None else count
    ids = np.array([site_params.NAME_IDS[n] for n in names], dtype=np.int32)
    kmax = 0 if eng.g_cnt is None else int(np.argmax(eng.g_cnt))
    L = 0
    for i in ids:
        n = ctypes.c_int()
        _lib.check(eng.lib.epx_named_len(eng.ctx, kmax, int(i), ctypes.byref(n)))
        L += n.value
    mean, m2 = np.full((count, L), np.nan), np.full((count, L), np.nan)
    S = 0
    if theta is not None:
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        assert theta.shape[0] == count and theta.shape[2] == eng.P
        S = theta.shape[1]
    n = ctypes.c_int()
    _lib.check(eng.lib.epx_named_moments(eng.ctx, k0, count, ids.ctypes.data_as(_lib.c_int32_p), len(names),
                                         _lib.dptr(theta), S, _lib.dptr(mean), _lib.dptr(m2), ctypes.byref(n)))
    return n.value, mean, m2


def _assert_site(model, D, ng, theta_k, names, mean, m2, what=''):
    mid, gauss, sg = _spec(model)
    n, hm, hv = site_params.named_moments_host(mid, D, ng, gauss, sg, theta_k, names)
    draws = site_params.named_draws(mid, D, ng, gauss, sg, theta_k, names)
    for name in names:
        assert np.shape(mean[name]) == np.shape(hm[name]) == np.shape(m2[name]), (what, name)
        np.testing.assert_allclose(mean[name], hm[name], rtol=RTOL, atol=1e-12 * np.abs(draws[name]).max(),
                                   err_msg='%s mean %s' % (what, name))
        np.testing.assert_allclose(m2[name], hv[name], rtol=RTOL, err_msg='%s m2 %s' % (what, name))


# ------------------------------------------------------------------ (a) injected draws, every model family
@pytest.mark.parametrize('model', ['m1b_sg', 'm2b_sg', 'm3b_sg', 'm4b_sg', 'm5b_sg', 'm1a_sg', 'm4a_sg'])
@pytest.mark.parametrize('D,chains,nkeep', [(1, 3, 7), (3, 4, 10), (21, 4, 25), (32, 4, 100)])
def test_injected_draws_match_the_host_moments(model, D, chains, nkeep):
    K, S = 5, chains * nkeep
    X, y, k_lim, _, _, d, P = _site_problem(model, D, 7, 300 + D, K=K)
    eng = HipEngine(model, X, y, k_lim)
    assert eng.P == P
    mid, gauss, sg = _spec(model)
    names = site_params.names(mid, gauss)
    theta = 0.5 * np.random.RandomState(7 + D).randn(K, S, P) + 0.3
    n, mean, m2 = eng.named_moments(names, theta=theta)                 # every name in one call
    assert n == S and len(mean) == len(m2) == K
    for k in range(K):
        _assert_site(model, D, 1, theta[k], names, mean[k], m2[k], 'all, site %d' % k)
    for name in names:                                                  # one name at a time: the same numbers
        _, m1, v1 = eng.named_moments([name], theta=theta)
        for k in range(K):
            _assert_site(model, D, 1, theta[k], [name], m1[k], v1[k], 'single, site %d' % k)
    _, ms, vs = eng.named_moments(names, k0=1, count=3, theta=theta[1:4])        # a sub-range
    for j in range(3):
        _assert_site(model, D, 1, theta[1 + j], names, ms[j], vs[j], 'range, site %d' % (1 + j))
    eng.close()


# ------------------------------------------------------------------ (b) means far from zero: the sums must be centred
@pytest.mark.parametrize('S', [21, 400])
def test_ill_conditioned_draws_need_the_centred_sum(S):
    D, K = 3, 2
    X, y, k_lim, _, _, d, P = _site_problem('m4b_sg', D, 7, 17, K=K)
    eng = HipEngine('m4b_sg', X, y, k_lim)
    rng = np.random.RandomState(S)
    theta = 0.5 * rng.randn(K, S, P)
    theta[:, :, 0] = 1e3 + 1e-2 * rng.randn(K, S)                       # mu_a
    theta[:, :, 2:2 + D] = 1e3 + 1e-2 * rng.randn(K, S, D)              # mu_b
    names = ['phi', 'mu_a', 'mu_b']
    _, mean, m2 = eng.named_moments(names, theta=theta)
    for k in range(K):
        _, hm, hv = site_params.named_moments_host(3, D, 1, False, True, theta[k], names)
        for name in names:
            print('S=%d site %d %s: mean err %.3e, m2 rel err %.3e' % (
                S, k, name, np.abs(mean[k][name] - hm[name]).max(), np.abs(m2[k][name] / hv[name] - 1).max()))
            np.testing.assert_allclose(mean[k][name], hm[name], rtol=RTOL)
            np.testing.assert_allclose(m2[k][name], hv[name], rtol=RTOL)
    eng.close()


# ------------------------------------------------------------------ (c) sites with several groups
@pytest.mark.parametrize('model,D,groups', [('m4b', 3, [[9], [8, 7, 9], [10, 6]]), ('m1b', 3, [[9], [8, 7, 9], [10, 6]]),
                                            # all names of this one are 352 elements: more than the workgroup's 256 threads
                                            ('m4b', 21, [[5], [4, 3, 4, 5, 3, 4]])])
def test_multi_group_sites_shapes_padding_and_own_coordinates(model, D, groups):
    S, K = 30, len(groups)
    X, y, k_lim, g_cnt, g_lim, _, _, d = _group_problem(model, D, groups, 23)
    eng = HipEngine(model, X, y, k_lim, g_cnt=g_cnt, g_lim=g_lim)
    mid, gauss, sg = _spec(model)
    names = site_params.names(mid, gauss)
    rng = np.random.RandomState(3)
    theta = np.full((K, S, eng.P), np.nan)                              # NaN behind every site's own coordinates
    for k in range(K):
        theta[k, :, :eng.site_P[k]] = 0.5 * rng.randn(S, eng.site_P[k])
    n, mean, m2 = eng.named_moments(names, theta=theta)
    for k in range(K):
        ng = int(g_cnt[k])
        assert mean[k]['alpha'].shape == (ng,) and mean[k]['eta'].shape == (ng,)
        assert mean[k]['beta'].shape == ((ng, D) if model == 'm4b' else (D,))
        assert all(np.all(np.isfinite(mean[k][nm])) and np.all(np.isfinite(m2[k][nm])) for nm in names)
        _assert_site(model, D, ng, theta[k, :, :eng.site_P[k]], names, mean[k], m2[k], 'site %d' % k)
        ln = ctypes.c_int()
        _lib.check(eng.lib.epx_named_len(eng.ctx, k, site_params.NAME_IDS['beta'], ctypes.byref(ln)))
        assert ln.value == (ng * D if model == 'm4b' else D)
    # the rows of the C interface: a name's block is sized by the largest site, exactly zero behind the site's own part
    for req in (['alpha', 'beta'] if model == 'm4b' else ['alpha', 'eta']), names:
        _, rm, rv = _raw(eng, req, theta)
        at = 0
        for name in req:
            per_site = [int(np.size(mean[k][name])) for k in range(K)]
            width = max(per_site)                                       # the block is sized by the largest site
            for k in range(K):
                own = per_site[k]
                # (another set of names is another split of the draws into slices: the sums agree to S 2^-53, not bit for bit)
                np.testing.assert_allclose(rm[k, at:at + own], np.ravel(mean[k][name]), rtol=1e-12, atol=1e-14)
                np.testing.assert_allclose(rv[k, at:at + own], np.ravel(m2[k][name]), rtol=1e-12)
                assert np.all(rm[k, at + own:at + width] == 0.0) and np.all(rv[k, at + own:at + width] == 0.0)
            at += width
        assert rm.shape == (K, at)
    eng.close()


# ------------------------------------------------------------------ (d) the sampler's own draws, (e) error paths
def test_sampler_draws_on_the_device_and_error_paths():
    D, K = 4, 6
    X, y, k_lim, Oms, mus, d, P = _site_problem('m4b_sg', D, 40, 41, K=K, tight=4.0)
    eng, _, _ = _engine_with_cavity('m4b_sg', X, y, k_lim, Oms, mus)
    names = site_params.names(3, False)
    with pytest.raises(_lib.EpxError, match='no draws yet'):           # (e) nothing sampled yet
        eng.named_moments(names)
    assert b'no draws yet' in eng.lib.epx_last_error()
    opts = HipEngine.sampler_opts(chains=4, iter=24, warmup=None, init='random')
    eng.sample_batch(np.arange(11, 11 + K, dtype=np.int64), opts)
    n, mean, m2 = _raw(eng, names)
    assert n == 48 and np.all(np.isfinite(mean)) and np.all(m2 >= 0)
    n2, mean2, m22 = _raw(eng, names)
    assert mean.tobytes() == mean2.tobytes() and m2.tobytes() == m22.tobytes()       # twice: the same bits
    draws = np.stack([np.ascontiguousarray(eng.get_draws(k, all_params=True)) for k in range(K)])
    n3, mean3, m23 = _raw(eng, names, draws)
    assert n3 == 48 and mean.tobytes() == mean3.tobytes() and m2.tobytes() == m23.tobytes()
    _, ms, vs = eng.named_moments(names, k0=2, count=3)                # a sub-range of the device draws
    for j in range(3):
        _assert_site('m4b_sg', D, 1, draws[2 + j], names, ms[j], vs[j], 'site %d' % (2 + j))
    eng.sample_batch(np.array([5, 6], dtype=np.int64), opts, k0=1, count=2)      # only sites 1, 2 are current now
    eng.named_moments(names, k0=1, count=2)
    with pytest.raises(_lib.EpxError, match='left draws of sites'):
        eng.named_moments(names)
    eng.close()
    X, y, k_lim, _, _, d, P = _site_problem('m1b_sg', 3, 7, 5, K=2)
    eng = HipEngine('m1b_sg', X, y, k_lim)
    with pytest.raises(_lib.EpxError, match='not defined'):            # (e) a name the model lacks
        eng.named_moments(['sigma_b'], theta=np.zeros((2, 8, P)))
    assert eng.lib.epx_last_error()
    ids = np.array([99], dtype=np.int32)
    out = np.zeros(4)
    assert eng.lib.epx_named_moments(eng.ctx, 0, 2, ids.ctypes.data_as(_lib.c_int32_p), 1, _lib.dptr(np.zeros((2, 8, P))),
                                     8, _lib.dptr(out), _lib.dptr(out), None) < 0
    eng.close()


# ------------------------------------------------------------------ (f) Master.mix_pred on the device
@pytest.mark.parametrize('J,K', [(4, 4), (5, 3)])
def test_master_mix_pred_on_the_device(J, K):
    D = 3
    conf = fit.configurations(J=J, D=D, K=K, npg=30, siter=40, run_ep=True, damp=0.4)
    M = fit.main('m4b', conf, ret_master=True)
    assert isinstance(M.engine, HipEngine)
    info = M.run(2, verbose=False, calc_moments=False, seed=5)
    assert info == 0
    pnames, pshapes, phiers = models.m4b(J, D, 30).get_param_definitions()
    pmaps = fit._create_pmaps(phiers, J, K, M._site_ng if K < J else None)
    ms, vs = M.mix_pred(pnames, pmaps, pshapes)
    assert ms[0].shape == (J,) and vs[1].shape == (J, D) and np.all(vs[0] > 0) and np.all(vs[1] > 0)
    mid, gauss, sg = _spec(M.model_name)
    recs = [site_params.named_moments_host(mid, D, int(M._site_ng[k]), gauss, sg,
                                           M.engine.get_draws(k, all_params=True)[:, :M.engine.site_P[k]] if K < J
                                           else M.engine.get_draws(k, all_params=True), list(pnames)) for k in range(K)]
    for i, p in enumerate(pnames):
        em, ev = combine_moments([r[0] for r in recs], [r[1][p] for r in recs], [r[2][p] for r in recs],
                                 pmaps[i], pshapes[i])
        np.testing.assert_allclose(ms[i], em, rtol=RTOL)
        np.testing.assert_allclose(vs[i], ev, rtol=RTOL)
