"""k_loo / k_psis_rows / epx_loo / epx_psis_rows / Master.loo on the device: leave-one-out cross-validation (PSIS-LOO, WAIC)
from draws in device memory, against loo.psis_host / loo.loo_host (NumPy) on the same inputs.  Need a real MI355X.

Tolerances (derived, not tuned):
  - the PSIS stage on IDENTICAL log-likelihoods: the host statement is evaluated in float64 and in np.longdouble; the
    device may differ from the float64 host by 100 x the largest |float64 - longdouble| of the output over the rows of
    the case (a different summation order, other log1p / expm1 / exp), floored at 1e-12 relative;
  - LPD, LL_MEAN, LL_M2 of epx_loo: test_gpu_predict's bounds (|d ll| <= 129 2^-53 A_i per term and more for the Gaussian
    family): rtol 1e-9 + atol 1e-10 max(1, A_i) for LPD and LL_MEAN, rtol 1e-9 for the centred LL_M2;
  - ELPD, KHAT, WESS of epx_loo inherit the rounding of ll: 10 x the largest change of psis_host over the rows under three
    random perturbations of ll within +-8 129 2^-53 A_i (10: worst case over random), floored at 1e-10.
Measured on an MI355X (largest error / bound over all cases): the PSIS stage stays below 6.7e-3 of its
bound, epx_loo below 4.2e-2 of the bound on ELPD, KHAT and WESS."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from epstan_amd import _lib, fit, loo, site_params             # noqa: E402
from epstan_amd.engine import HipEngine, MODEL_IDS, is_gauss    # noqa: E402
from test_gpu_parity import _site_problem, _engine_with_cavity, _group_problem   # noqa: E402
from test_gpu_predict import _scale, _close, RTOL               # noqa: E402

LPD, LL_MEAN, LL_M2, ELPD, KHAT, WESS = (loo.LO_LPD, loo.LO_LL_MEAN, loo.LO_LL_M2, loo.LO_ELPD, loo.LO_KHAT,
                                         loo.LO_WESS)
PSIS_NAMES = ('ELPD', 'KHAT', 'WESS')


def _spec(model):
    return MODEL_IDS[model] % 5, is_gauss(model)


# ------------------------------------------------------------------ (a) the PSIS stage on identical inputs
def _tied(S):
    """Three tied levels, 60 % / 30 % / 10 % of the draws (S = 50: the 30 / 15 / 5 of the host test)."""
    n1, n2 = (3 * S) // 5, (3 * S) // 10
    return np.concatenate([np.full(n1, -0.1), np.full(n2, -0.2), np.full(S - n1 - n2, -3.0)])


def _psis_inputs(S, seed):
    """37 rows: 17 Gaussian rows (the analytic case of the host test), 18 Bernoulli rows, a constant and a tied one."""
    rng = np.random.RandomState(seed)
    rows = []
    for i in range(17):
        th = 0.2 + 0.5 * np.random.RandomState(1000 * seed + i).randn(S)
        rows.append(-0.5 * np.log(2 * np.pi) - 0.5 * np.square(0.7 - th))
    for i in range(18):
        f, y = 3.0 * rng.randn(S), float(i % 2)
        rows.append(y * f - (np.maximum(f, 0.0) + np.log1p(np.exp(-np.abs(f)))))
    rows.append(np.full(S, -0.3))
    rows.append(_tied(S))
    return np.ascontiguousarray(np.stack(rows))


@pytest.fixture(scope='module')
def eng0():
    X, y, k_lim, _, _, _, _ = _site_problem('m1b_sg', 2, 7, 5, K=2)
    eng = HipEngine('m1b_sg', X, y, k_lim)
    yield eng
    eng.close()


def _psis_check(got, ll, what):
    """Device (n, 3) against psis_host on the same ll; returns the largest error / bound."""
    host = loo.psis_host(ll)
    with np.errstate(all='ignore'):
        wide = loo.psis_host(ll.astype(np.longdouble))
    raw = np.isinf(host[:, 1])
    assert np.array_equal(raw, np.isinf(wide[:, 1].astype(np.float64))), what
    assert np.array_equal(raw, np.isposinf(got[:, 1])), what + ': not-smoothed rows are exactly +inf in KHAT'
    assert not np.any(np.isnan(got)), what
    worst = 0.0
    for c, name in enumerate(PSIS_NAMES):
        use = ~raw if c == 1 else np.ones(len(raw), dtype=bool)
        if not use.any():
            continue
        ref = float(np.abs((host[use, c] - wide[use, c]).astype(np.float64)).max())
        err = np.abs(got[use, c] - host[use, c])
        bound = np.maximum(100.0 * ref, 1e-12 * np.abs(host[use, c]))
        ratio = float((err / bound).max())
        print('%s %s: largest error %.3e, float64 - longdouble %.3e, largest error / bound %.3e'
              % (what, name, err.max(), ref, ratio))
        assert np.all(err <= bound), '%s %s' % (what, name)
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize('S', [24, 25, 33, 50, 100, 225, 226, 400, 2000])
def test_psis_rows_match_the_host_on_identical_inputs(eng0, S):
    ll = _psis_inputs(S, S)
    assert ll.shape == (37, S)
    got = eng0.psis_rows(ll)
    assert got.shape == (37, 3)
    assert got.tobytes() == eng0.psis_rows(ll).tobytes()                # twice: the same bytes
    _psis_check(got, ll, 'S=%d' % S)
    host = loo.psis_host(ll)
    assert np.all(np.isinf(host[-2:, 1]))                               # the constant and the tied row
    np.testing.assert_allclose(got[-2, 0], -0.3, rtol=1e-13)
    np.testing.assert_allclose(got[-2, 2], S, rtol=1e-12)
    if S == 24:
        assert np.all(np.isinf(host[:, 1]))                             # M = 4: nothing is smoothed
    if S == 25:
        assert np.any(np.isfinite(host[:, 1]))                          # M = 5: the first smoothed length
    bad = ll.copy()
    bad[3, S // 2], bad[5, 0], bad[36, S - 1] = np.nan, np.inf, -np.inf
    gb = eng0.psis_rows(bad)
    hit = np.zeros(37, dtype=bool)
    hit[[3, 5, 36]] = True
    assert np.all(np.isnan(gb[hit])) and gb[~hit].tobytes() == got[~hit].tobytes()


def test_psis_rows_bad_arguments_are_errors(eng0):
    out = np.zeros((1, 3))
    ll = np.zeros((1, 4))
    assert eng0.lib.epx_psis_rows(0, 1, 0, _lib.dptr(ll), _lib.dptr(out)) != 0
    assert eng0.lib.epx_psis_rows(0, -1, 4, _lib.dptr(ll), _lib.dptr(out)) != 0
    assert eng0.lib.epx_psis_rows(0, 1, 4, None, _lib.dptr(out)) != 0
    assert eng0.lib.epx_psis_rows(99, 1, 4, _lib.dptr(ll), _lib.dptr(out)) != 0
    assert eng0.psis_rows(np.zeros((0, 5))).shape == (0, 3)
    assert eng0.psis_rows(np.full((3, 1), -2.0)).tolist() == [[-2.0, np.inf, 1.0]] * 3     # S = 1


# ------------------------------------------------------------------ (b) epx_loo with injected draws, every family
def _assert_loo_site(model, D, ng, theta_k, X, group, y, got, eng, what, worst=None):
    """The rows of ONE site against loo_host on the same draws."""
    mid, gauss = _spec(model)
    n = X.shape[0]
    group = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group)
    yf = np.asarray(y, dtype=np.float64)
    ll = loo.loglik_host(mid, D, ng, gauss, theta_k, X, group, yf)
    exp = loo.loo_rows(ll)
    A = np.maximum(1.0, _scale(model, D, ng, theta_k, X, group))
    assert got.shape == exp.shape == (n, 6)
    assert np.all(np.isfinite(got[:, [LPD, LL_MEAN, LL_M2, ELPD, WESS]])), what
    _close(got[:, LPD], exp[:, LPD], RTOL, 1e-10 * A, what + ' LPD')
    _close(got[:, LL_MEAN], exp[:, LL_MEAN], RTOL, 1e-10 * A, what + ' LL_MEAN')
    _close(got[:, LL_M2], exp[:, LL_M2], RTOL, 0.0, what + ' LL_M2')
    # the PSIS columns: how far the rounding of ll moves the host's own result
    rng = np.random.RandomState(n + 31 * D)
    delta = np.zeros(3)
    raw = np.isinf(exp[:, KHAT])
    for _ in range(3):
        moved = loo.psis_host(ll + (2 * rng.rand(*ll.shape) - 1) * (8 * 129 * 2.0 ** -53) * A[:, None])
        same = np.isinf(moved[:, 1]) == raw                              # (tied draws, e.g. a chain that stood still: the
        if not same.any():                                               # perturbation breaks the tie and the decision of
            continue                                                     # step 5 with it -- such a row sets no scale)
        with np.errstate(invalid='ignore'):
            change = np.where(np.isinf(moved[same]), 0.0, np.abs(moved[same] - exp[same, ELPD:]))
        delta = np.maximum(delta, change.max(axis=0))
    bound = np.maximum(10.0 * delta, 1e-10)
    assert np.array_equal(np.isposinf(got[:, KHAT]), raw), what + ': not-smoothed rows'
    alone = eng.psis_rows(ll)                                            # the PSIS stage alone on the host's ll
    assert np.array_equal(np.isposinf(alone[:, 1]), raw), what
    for c, name in enumerate(PSIS_NAMES):
        use = ~raw if c == 1 else np.ones(n, dtype=bool)
        if not use.any():
            continue
        err = float(np.abs(got[use, ELPD + c] - exp[use, ELPD + c]).max())
        err2 = float(np.abs(got[use, ELPD + c] - alone[use, c]).max())
        print('%s %s: largest error %.3e (against epx_psis_rows on the host\'s ll %.3e), bound %.3e, error / bound %.3e'
              % (what, name, err, err2, bound[c], max(err, err2) / bound[c]))
        assert err <= bound[c] and err2 <= bound[c], '%s %s' % (what, name)
        if worst is not None:
            worst.append(max(err, err2) / bound[c])


ROWS = np.array([3, 16, 17, 33])             # below a tile, a full tile, one past it, three tiles


def _rows_problem(model, D, seed):
    rng = np.random.RandomState(seed)
    k_lim = np.concatenate(([0], np.cumsum(ROWS)))
    N = int(k_lim[-1])
    X = 1.5 * rng.randn(N, D)
    y = 0.4 + rng.randn(N) if is_gauss(model) else (rng.rand(N) < 0.5).astype(int)
    return X, y, k_lim


@pytest.mark.parametrize('model', ['m1b_sg', 'm4b_sg', 'm5b_sg', 'm1a_sg', 'm4a_sg'])
@pytest.mark.parametrize('D,S', [(1, 25), (3, 33), (32, 100), (128, 226)])
def test_injected_draws_match_the_host_loo(model, D, S):
    K = len(ROWS)
    X, y, k_lim = _rows_problem(model, D, 300 + D)
    eng = HipEngine(model, X, y, k_lim)
    rng = np.random.RandomState(7 + D)
    theta = 0.5 * rng.randn(K, S, eng.P) + 0.3
    got, n = eng.loo(theta=theta, with_n=True)
    assert n == S and got.shape == (int(k_lim[-1]), 6)
    assert got.tobytes() == eng.loo(theta=theta).tobytes()              # twice: the same bytes
    for k in range(K):
        sl = slice(k_lim[k], k_lim[k + 1])
        _assert_loo_site(model, D, 1, theta[k], X[sl], None, y[sl], got[sl], eng, 'site %d' % k)
    # LPD is EPX_PR_LPD of the row, bit for bit: one row-tile walk forms the log-likelihoods of both (csrc/predict_tile.h)
    pr = eng.predict(X, k_lim, y=np.asarray(y, dtype=np.float64), theta=theta)
    print('largest |LO_LPD - PR_LPD|: %.3e' % np.abs(got[:, LPD] - pr[:, site_params.PR_LPD]).max())
    assert got[:, LPD].tobytes() == pr[:, site_params.PR_LPD].tobytes()
    sub = eng.loo(k0=1, count=2, theta=theta[1:3])                      # a sub-range: the same rows, the same bytes
    assert sub.tobytes() == got[k_lim[1]:k_lim[3]].tobytes()
    eng.close()


@pytest.mark.parametrize('model,S', [('m4b_sg', 226), ('m4a_sg', 2000)])
def test_the_workspace_tile_gives_the_bits_of_the_lds_tile(model, S, monkeypatch):
    """S = 2000: 16 x S log-likelihoods are beyond the LDS; and the LDS budget taken away at a length that fits."""
    D, K = 3, len(ROWS)
    X, y, k_lim = _rows_problem(model, D, 11)
    eng = HipEngine(model, X, y, k_lim)
    theta = 0.5 * np.random.RandomState(S).randn(K, S, eng.P) + 0.3
    got = eng.loo(theta=theta)
    if S == 226:
        monkeypatch.setenv('EPX_LOO_LDS_BYTES', '0')
        assert eng.loo(theta=theta).tobytes() == got.tobytes()
        monkeypatch.setenv('EPX_LOO_LDS_BYTES', '70000')                # fewer tiles per work item
        assert eng.loo(theta=theta).tobytes() == got.tobytes()
    for k in (0, 2):
        sl = slice(k_lim[k], k_lim[k + 1])
        _assert_loo_site(model, D, 1, theta[k], X[sl], None, y[sl], got[sl], eng, 'S=%d site %d' % (S, k))
    eng.close()


# ------------------------------------------------------------------ (c) sites with several groups
@pytest.mark.parametrize('model', ['m4b', 'm1b'])
def test_multi_group_sites_read_their_own_coordinates(model):
    D, S, groups = 3, 30, [[9], [8, 7, 9], [10, 6]]
    K = len(groups)
    X, y, k_lim, g_cnt, g_lim, _, _, d = _group_problem(model, D, groups, 23)
    eng = HipEngine(model, X, y, k_lim, g_cnt=g_cnt, g_lim=g_lim)
    rng = np.random.RandomState(3)
    theta = np.full((K, S, eng.P), np.nan)                              # NaN behind every site's own coordinates
    for k in range(K):
        theta[k, :, :eng.site_P[k]] = 0.5 * rng.randn(S, eng.site_P[k]) + 0.3
    got = eng.loo(theta=theta)
    assert np.all(np.isfinite(np.delete(got, KHAT, axis=1)))
    assert not np.any(np.isnan(got[:, KHAT]))
    for k in range(K):
        sl = slice(k_lim[k], k_lim[k + 1])
        group = np.concatenate([np.full(n, g) for g, n in enumerate(groups[k])])
        _assert_loo_site(model, D, int(g_cnt[k]), theta[k, :, :eng.site_P[k]], X[sl], group, y[sl], got[sl], eng,
                         'site %d' % k)
    # a sub-range starts at its own first group: the same bytes as those rows of the whole range
    sub = eng.loo(k0=1, count=2, theta=theta[1:3])
    assert sub.tobytes() == got[k_lim[1]:k_lim[3]].tobytes()
    eng.close()


# ------------------------------------------------------------------ (d) saturated logits
def test_saturated_logits_give_finite_results():
    D, K, S = 2, 2, 21
    X, y, k_lim, _, _, d, P = _site_problem('m1b_sg', D, 7, 5, K=K)
    eng = HipEngine('m1b_sg', X, y, k_lim)
    theta = np.zeros((K, S, P))                                         # [log sigma_a = 0, beta = 0 | eta]: f = eta
    theta[0, :, -1], theta[1, :, -1] = 750.0, -750.0
    got = eng.loo(theta=theta)
    print(got)
    assert not np.any(np.isnan(got))
    f = np.repeat([750.0, -750.0], 7)
    wrong = (y == 0) == (f > 0)                                         # y = 0 at f = 750, y = 1 at f = -750
    assert wrong.any() and (~wrong).any()
    np.testing.assert_allclose(got[wrong][:, [LPD, ELPD]], -750.0, rtol=1e-9)
    np.testing.assert_allclose(got[~wrong][:, [LPD, ELPD]], 0.0, atol=1e-300)
    assert np.all(np.isposinf(got[:, KHAT]))
    np.testing.assert_allclose(got[:, WESS], S, rtol=1e-12)
    assert np.all(got[:, LL_M2] == 0.0)
    eng.close()


def test_a_non_finite_log_likelihood_gives_six_nans():
    D, K, S = 2, 2, 40
    X, y, k_lim, _, _, d, P = _site_problem('m4a_sg', D, 7, 5, K=K)
    eng = HipEngine('m4a_sg', X, y, k_lim)
    theta = 0.3 * np.random.RandomState(0).randn(K, S, P)
    good = eng.loo(theta=theta)
    theta[1, 17, 0] = np.inf                                            # sigma = inf in one draw of site 1
    got = eng.loo(theta=theta)
    assert np.all(np.isnan(got[7:])) and got[:7].tobytes() == good[:7].tobytes()
    eng.close()


# ------------------------------------------------------------------ (e) the sampler's own draws, repeatability, errors
def test_sampler_draws_on_the_device_and_repeatability():
    D, K = 4, 6
    X, y, k_lim, Oms, mus, d, P = _site_problem('m4b_sg', D, 40, 41, K=K, tight=4.0)
    eng, _, _ = _engine_with_cavity('m4b_sg', X, y, k_lim, Oms, mus)
    with pytest.raises(_lib.EpxError, match='no draws yet'):            # nothing sampled yet
        eng.loo()
    opts = HipEngine.sampler_opts(chains=4, iter=24, warmup=None, init='random')
    eng.sample_batch(np.arange(11, 11 + K, dtype=np.int64), opts)
    got, n = eng.loo(with_n=True)
    assert n == 48 and got.shape == (K * 40, 6)
    assert got.tobytes() == eng.loo().tobytes()                         # twice: the same bytes
    draws = np.stack([np.ascontiguousarray(eng.get_draws(k, all_params=True)) for k in range(K)])
    assert got.tobytes() == eng.loo(theta=draws).tobytes()
    for k in range(K):
        sl = slice(k_lim[k], k_lim[k + 1])
        _assert_loo_site('m4b_sg', D, 1, draws[k], X[sl], None, y[sl], got[sl], eng, 'site %d' % k)
    assert eng.loo(k0=2, count=3).tobytes() == got[k_lim[2]:k_lim[5]].tobytes()
    eng.sample_batch(np.array([5, 6], dtype=np.int64), opts, k0=1, count=2)     # only sites 1, 2 are current now
    assert eng.loo(k0=1, count=2).shape == (80, 6)
    with pytest.raises(_lib.EpxError, match='left draws of sites'):
        eng.loo()
    for k0, count in ((-1, 2), (5, 2), (0, 0), (6, 1)):
        with pytest.raises(_lib.EpxError, match='site range'):
            eng.loo(k0=k0, count=count, theta=np.zeros((max(count, 0), 8, P)))
    out = np.zeros((40, 6))
    assert eng.lib.epx_loo(eng.ctx, 0, 1, _lib.dptr(np.zeros((1, 8, P))), 0, _lib.dptr(out), None) != 0    # S < 1
    assert b'S = 0' in eng.lib.epx_last_error()
    eng.close()


# ------------------------------------------------------------------ (f) Master.loo on the device
@pytest.mark.parametrize('J,K', [(4, 4), (5, 3)])
def test_master_loo_on_the_device(J, K):
    D = 3
    conf = fit.configurations(J=J, D=D, K=K, npg=30, siter=40, run_ep=True, damp=0.4)
    M = fit.main('m4b', conf, ret_master=True)
    assert isinstance(M.engine, HipEngine)
    with pytest.raises(RuntimeError, match='before at least one iteration'):
        M.loo()
    assert M.run(2, verbose=False, calc_moments=False, seed=5) == 0
    multi = not M.model_name.endswith('_sg')
    assert multi == (K < J)
    res = M.loo()
    S = M.engine.num_draws()
    N = M.N
    assert res['n'] == S
    for key in ('lpd', 'elpd_loo_i', 'p_loo_i', 'elpd_waic_i', 'p_waic_i', 'khat', 'wess', 'll_mean'):
        assert res[key].shape == (N,), key
    for key in ('site_elpd_loo', 'site_p_loo', 'site_elpd_waic', 'site_p_waic', 'site_lpd'):
        assert res[key].shape == (K,), key
    assert res['p_loo'] > 0 and res['p_waic'] > 0 and res['elpd_loo'] < res['lpd'].sum()
    np.testing.assert_allclose(res['site_elpd_loo'].sum(), res['elpd_loo'], rtol=1e-12)
    assert res['n_bad'] == int(np.count_nonzero(res['khat'] > res['khat_threshold']))
    assert res['khat_threshold'] == min(1 - 1 / np.log10(S), 0.7)
    if res['worst'] is not None:
        k, i = res['worst']
        assert res['khat'][M.k_lim[k] + i] == res['khat'][np.isfinite(res['khat'])].max()
    got = np.stack([res['lpd'], res['ll_mean'], res['p_waic_i'] * (S - 1), res['elpd_loo_i'], res['khat'], res['wess']],
                   axis=1)
    j_ind = np.asarray(M.A_n['j_ind']) if multi else None
    for k in range(K):
        sl = slice(M.k_lim[k], M.k_lim[k + 1])
        theta_k = M.engine.get_draws(k, all_params=True)
        theta_k = theta_k[:, :M.engine.site_P[k]] if multi else theta_k
        _assert_loo_site(M.model_name, D, int(M._site_ng[k]), theta_k, M.X[sl], j_ind[sl] - 1 if multi else None,
                         M.y[sl], got[sl], M.engine, 'site %d' % k)
