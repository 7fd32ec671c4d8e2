"""The two routes to `Master`'s seven draw queries on ONE fit: the device route `Master` takes as built, and the host route
(`draw_queries.HostDraws`) forced over the same `HipEngine`, so that both read the same device draws.  Need a real MI355X.

No tolerance is new: every query is held to what its own device test allows between the device and the host functions,
through that test's own helper where it has one (cited at each use)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from epstan_amd import fit, loo, models, site_params                                        # noqa: E402
from epstan_amd.diagnostics import DG_NAMES, RD_NAMES                                        # noqa: E402
from epstan_amd.draw_queries import HostDraws, QUERIES                                       # noqa: E402
from epstan_amd.engine import HipEngine                                                      # noqa: E402
from test_gpu_draw_diag import _close as _diag_close, RTOL as DIAG_RTOL                      # noqa: E402
from test_gpu_loo import _assert_loo_site                                                    # noqa: E402
from test_gpu_named_moments import RTOL as MOMENTS_RTOL                                      # noqa: E402
from test_gpu_newgroup import _assert_close as _newgroup_close                               # noqa: E402
from test_gpu_predict import _close, _scale, RTOL as PREDICT_RTOL                            # noqa: E402
from test_gpu_quantiles import _quantile_bound, PROBS, RTOL as QUANTILES_RTOL               # noqa: E402
from test_gpu_rank_diag import _close as _rank_close, RTOL as RANK_RTOL                     # noqa: E402

J, K, D = 4, 2, 2


class _Spy(object):
    """Counts the calls of QUERIES that reach `target`."""

    def __init__(self, target):
        self.target, self.calls = target, []

    def __getattr__(self, name):
        if name not in QUERIES:
            raise AttributeError(name)
        self.calls.append(name)
        return getattr(self.target, name)


@pytest.fixture(scope='module')
def fitted():
    conf = fit.configurations(J=J, D=D, K=K, npg=30, siter=40, chains=4, run_ep=True, damp=0.4)
    M = fit.main('m4b', conf, ret_master=True)
    assert isinstance(M.engine, HipEngine) and M._queries.host.engine is M.engine and isinstance(M._queries.host, HostDraws)
    assert M.run(1, verbose=False, calc_moments=False, seed=5) == 0
    return M


@pytest.fixture(scope='module')
def both(fitted):
    """route(call) -> (the device route's result, the host route's) of call(M); every route is checked to have answered
    through its own side only."""
    M, resolver = fitted, fitted._queries

    def route(call, names):
        dev = call(M)
        spy = M._queries = _Spy(resolver.host)
        try:
            host = call(M)
        finally:
            M._queries = resolver
        assert sorted(set(spy.calls)) == sorted(names), spy.calls
        return dev, host
    return route


def _draws(M, names):
    mid, gauss, sg = M._site_spec()
    return [site_params.named_draws(mid, D, int(M._site_ng[k]), gauss, sg,
                                    np.ascontiguousarray(M.engine.get_draws(k, all_params=True)), names) for k in range(K)]


def test_mix_pred(fitted, both):
    pnames, pshapes, phiers = models.m4b(J, D, 30).get_param_definitions()
    pmaps = fit._create_pmaps(phiers, J, K, fitted._site_ng)
    (dm, dv), (hm, hv) = both(lambda M: M.mix_pred(pnames, pmaps, pshapes), ['named_moments'])
    for i in range(len(pnames)):
        np.testing.assert_allclose(dm[i], hm[i], rtol=MOMENTS_RTOL)            # test_gpu_named_moments.py:206
        np.testing.assert_allclose(dv[i], hv[i], rtol=MOMENTS_RTOL)            # test_gpu_named_moments.py:207


def test_mix_quantiles(fitted, both):
    pnames, pshapes, phiers = models.m4b(J, D, 30).get_param_definitions()
    pmaps = fit._create_pmaps(phiers, J, K, fitted._site_ng)
    shared = ['phi', 'sigma_a', 'mu_b']
    draws = _draws(fitted, list(pnames) + shared)
    dev, host = both(lambda M: M.mix_quantiles(pnames, smap=pmaps, param_shapes=pshapes), ['named_order_stats'])
    for name, mp, dq, hq in zip(pnames, pmaps, dev, host):
        for k in range(K):
            at = (slice(None),) + (mp[k] if isinstance(mp[k], tuple) else (mp[k],))
            np.testing.assert_allclose(dq[at], hq[at], rtol=QUANTILES_RTOL,     # test_gpu_quantiles.py:333
                                       atol=1e-12 * np.abs(draws[k][name]).max())
    dev, host = both(lambda M: M.mix_quantiles(shared, probs=PROBS), ['pooled_count_pass'])
    for name, dq, hq in zip(shared, dev, host):
        _, bound = _quantile_bound(np.concatenate([draws[k][name] for k in range(K)]), PROBS)
        print('%s: pooled quantiles, largest difference / bound %.3g' % (name, (np.abs(dq - hq) / bound).max()))
        assert dq.shape == hq.shape and np.all(np.abs(dq - hq) <= bound), name   # test_gpu_quantiles.py:342


def test_predict(fitted, both):
    M = fitted
    j_ind = np.asarray(M.A_n['j_ind'])
    dev, host = both(lambda M: M.predict(M.X, site_sizes=M.Nk, j_ind=j_ind, y_new=M.y), ['predict'])
    assert dev['n'] == host['n']
    for k in range(K):
        sl = slice(M.k_lim[k], M.k_lim[k + 1])
        A = np.maximum(1.0, _scale(M.model_name, D, int(M._site_ng[k]), M.engine.get_draws(k, all_params=True), M.X[sl],
                                   j_ind[sl] - 1))
        what = 'site %d' % k                                                    # test_gpu_predict.py:54-61
        _close(dev['mean'][sl], host['mean'][sl], PREDICT_RTOL, 1e-12 * A, what + ' MEAN')
        _close(dev['f_mean'][sl], host['f_mean'][sl], PREDICT_RTOL, 1e-12 * A, what + ' F_MEAN')
        _close(dev['f_var'][sl], host['f_var'][sl], PREDICT_RTOL, 0.0, what + ' F_M2')
        _close(dev['lpd'][sl], host['lpd'][sl], PREDICT_RTOL, 1e-10 * A, what + ' LPD')
    dev, host = both(lambda M: M.predict(M.X, site_sizes=M.Nk, j_ind=j_ind), ['predict'])
    assert dev['lpd'] is None and host['lpd'] is None
    _close(dev['f_var'], host['f_var'], PREDICT_RTOL, 0.0, 'without responses F_M2')


def test_predict_new_group(fitted, both):
    rng = np.random.RandomState(J)
    n, R = 40, 2
    Xn = rng.randn(n, D)
    group = rng.permutation(np.repeat([31, 2, 500000], [20, 3, 17]))
    yn = (rng.rand(n) < 0.5).astype(int)
    dev, host = both(lambda M: M.predict_new_group(Xn, group, y_new=yn, R=R, seed=77), ['predict_new_group'])
    phi = np.stack([np.ascontiguousarray(fitted.engine.get_draws(k)) for k in range(K)])
    N = K * fitted.engine.num_draws() * R

    def record(res):
        return np.stack([res['mean'], res['f_mean'], res['f_var'] * (N - 1), res['lpd']], axis=1), res['group_lpd'], res['n']
    assert list(dev['groups']) == list(host['groups']) == [2, 31, 500000] and dev['n'] == N
    _newgroup_close('m4b_sg', D, phi, Xn, np.searchsorted(dev['groups'], group), yn, record(dev), record(host),
                    'device route against host route')                          # test_gpu_newgroup.py:362


def test_loo(fitted, both):
    M = fitted
    dev, host = both(lambda M: M.loo(), ['loo'])
    S = M.engine.num_draws()
    assert dev['n'] == host['n'] == S
    mid, gauss, _ = M._site_spec()
    j_ind = np.asarray(M.A_n['j_ind'])
    got = np.stack([dev['lpd'], dev['ll_mean'], dev['p_waic_i'] * (S - 1), dev['elpd_loo_i'], dev['khat'], dev['wess']],
                   axis=1)
    for k in range(K):
        sl = slice(M.k_lim[k], M.k_lim[k + 1])
        theta_k = M.engine.get_draws(k, all_params=True)
        # the host route's record IS loo_host on these draws, which the device test's helper holds the device to
        exp = loo.loo_host(mid, D, int(M._site_ng[k]), gauss, theta_k, M.X[sl], j_ind[sl] - 1, M.y[sl])
        for key, col in (('lpd', loo.LO_LPD), ('ll_mean', loo.LO_LL_MEAN), ('elpd_loo_i', loo.LO_ELPD),
                         ('khat', loo.LO_KHAT), ('wess', loo.LO_WESS)):
            np.testing.assert_array_equal(host[key][sl], exp[:, col])
        np.testing.assert_allclose(host['p_waic_i'][sl], exp[:, loo.LO_LL_M2] / (S - 1), rtol=1e-15)
        _assert_loo_site(M.model_name, D, int(M._site_ng[k]), theta_k, M.X[sl], j_ind[sl] - 1, M.y[sl], got[sl], M.engine,
                         'site %d' % k)                                         # test_gpu_loo.py:342


def test_diagnostics(fitted, both):
    dev, host = both(lambda M: M.diagnostics(), ['draw_diagnostics'])
    np.testing.assert_array_equal(dev['n'], host['n'])
    for k in range(K):                                                          # test_gpu_draw_diag.py:227
        _diag_close(np.stack([dev[name][k] for name in DG_NAMES], axis=1),
                    np.stack([host[name][k] for name in DG_NAMES], axis=1), DIAG_RTOL, 'site %d' % k)


def test_rank_diagnostics(fitted, both):
    dev, host = both(lambda M: M.diagnostics(rank=True), ['draw_diagnostics', 'draw_rank_diagnostics'])
    for k in range(K):                                                          # test_gpu_rank_diag.py:216
        _rank_close(np.stack([dev[name][k] for name in RD_NAMES], axis=1),
                    np.stack([host[name][k] for name in RD_NAMES], axis=1), RANK_RTOL, 'site %d' % k)
