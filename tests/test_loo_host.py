"""loo.py, the NumPy / SciPy statement of leave-one-out cross-validation (include/epx.h, enum epx_loo), anchored to things
outside itself -- the generalised Pareto distribution's own quantiles, a Gaussian case with a closed form -- and
`Master.loo` on the CPU oracle engine.  CPU only."""

import numpy as np
import pytest
from scipy.stats import genpareto

from epstan_amd import fit, loo
from epstan_amd.method import Master
from oracle.engine_oracle import OracleEngine


def factory(model, X, y, k_lim, **groups):
    return OracleEngine(model, X, y, k_lim, **groups)


# ------------------------------------------------------------------ the fit
@pytest.mark.parametrize('M', [60, 95])
@pytest.mark.parametrize('k', [-0.3, 1e-4, 0.5, 0.9])
def test_gpd_fit_recovers_the_distribution_from_its_quantiles(M, k):
    """(the largest deviation is 0.049, at k = -0.3, M = 60; M = 20 does not meet 0.05)"""
    x = genpareto.ppf((np.arange(1, M + 1) - 0.5) / M, k)
    khat, sigma = loo.gpd_fit(x)
    raw = (khat * (M + 10) - 5) / M                      # the prior undone
    print('M=%d k=%g: k error %.4f, sigma error %.4f' % (M, k, raw - k, sigma - 1))
    assert abs(raw - k) < 0.05 and abs(sigma - 1) < 0.05


def test_tail_length_is_integer_arithmetic():
    for S in list(range(1, 3000)) + [7281, 10 ** 6, 10 ** 6 + 1]:
        assert loo.tail_length(S) == min(S // 5, int(np.ceil(3 * np.sqrt(np.longdouble(S))))), S
    assert [loo.tail_length(S) for S in (24, 25, 100, 225, 226, 400)] == [4, 5, 20, 45, 45, 60]


# ------------------------------------------------------------------ a case with a closed form
def test_analytic_gaussian_case():
    """ll_s = log N(y | theta_s, 1), theta ~ N(m, s^2): the leave-one-out predictive density of y is that of
    N(m, s^2) exp(+(y - theta)^2 / 2) normalised, a normal with variance s^2 / (1 - s^2), whence the value below.
    Measured: largest |ELPD - exact| 0.0200, mean error -3.8e-5 (standard error 1.2e-3), KHAT in [0.12, 0.56]."""
    y, m, s, S = 0.7, 0.2, 0.5, 4000
    exact = -0.5 * np.log(2 * np.pi) + 0.5 * np.log(1 - s * s) - (y - m) ** 2 / (2 * (1 - s * s))
    ll = np.stack([-0.5 * np.log(2 * np.pi) - 0.5 * np.square(y - (m + s * np.random.RandomState(seed).randn(S)))
                   for seed in range(40)])
    out = loo.psis_host(ll)
    err = out[:, 0] - exact
    print('largest |ELPD - exact| %.4f, mean error %.2e, KHAT in [%.2f, %.2f]'
          % (np.abs(err).max(), err.mean(), out[:, 1].min(), out[:, 1].max()))
    assert np.abs(err).max() < 0.04
    assert abs(err.mean()) < 0.005
    assert np.all((out[:, 1] > 0.05) & (out[:, 1] < 0.7))
    assert np.all((out[:, 2] > 1) & (out[:, 2] <= S))


# ------------------------------------------------------------------ edges
def test_constant_and_tied_rows_are_not_smoothed():
    out = loo.psis_host(np.full((1, 50), -0.3))[0]
    assert abs(out[0] + 0.3) <= 1e-14 and out[1] == np.inf
    np.testing.assert_allclose(out[2], 50, rtol=1e-13)
    tied = np.concatenate([np.full(30, -0.1), np.full(15, -0.2), np.full(5, -3.0)])
    out = loo.psis_host(tied[None, :])[0]
    assert out[1] == np.inf                                              # x_q = 0
    w = np.exp(-tied) / np.exp(-tied).sum()                              # the raw ratios
    np.testing.assert_allclose(out[0], np.log((w * np.exp(tied)).sum()), rtol=1e-13)
    np.testing.assert_allclose(out[2], 1 / np.square(w).sum(), rtol=1e-13)


def test_the_first_smoothed_length_is_25():
    rng = np.random.RandomState(1)
    for _ in range(5):
        ll = -np.square(rng.randn(25))
        assert loo.psis_host(ll[None, :24])[0, 1] == np.inf              # M = 4
        assert np.isfinite(loo.psis_host(ll[None, :])[0, 1])             # M = 5
    assert loo.psis_host(np.array([[-2.0]])).tolist() == [[-2.0, np.inf, 1.0]]


def test_a_nan_gives_six_nans_and_s_1_a_zero_m2():
    ll = -np.square(np.random.RandomState(0).randn(3, 40))
    ll[1, 7] = np.nan
    out = loo.loo_rows(ll)
    assert np.all(np.isnan(out[1])) and np.all(np.isfinite(out[[0, 2]]))
    ll[1, 7] = -np.inf
    assert np.all(np.isnan(loo.loo_rows(ll)[1]))
    one = loo.loo_rows(np.array([[-1.5]]))[0]
    assert one.tolist() == [-1.5, -1.5, 0.0, -1.5, np.inf, 1.0]


def test_permuting_the_draws_changes_nothing_but_rounding():
    rng = np.random.RandomState(5)
    ll = -0.5 * np.square(0.7 - 0.2 - 0.5 * rng.randn(6, 400)) - 0.9
    a = loo.psis_host(ll)
    b = loo.psis_host(ll[:, rng.permutation(400)])
    assert np.all(np.isfinite(a))
    np.testing.assert_allclose(b[:, 0], a[:, 0], rtol=1e-13)
    np.testing.assert_allclose(b[:, 1:], a[:, 1:], rtol=1e-10)


def test_long_double_agrees_with_double():
    ll = -np.square(np.random.RandomState(2).randn(5, 226))
    a, b = loo.psis_host(ll), loo.psis_host(ll.astype(np.longdouble))
    assert b.dtype == np.longdouble
    np.testing.assert_allclose(a, b.astype(np.float64), rtol=1e-11)


def test_summarise_totals_sites_and_bad_rows():
    rng = np.random.RandomState(3)
    S, k_lim = 100, np.array([0, 4, 9, 12])
    rec = np.column_stack([-1 - rng.rand(12), -1.5 - rng.rand(12), 30 * rng.rand(12), -1.2 - rng.rand(12),
                           rng.rand(12), 50 * rng.rand(12)])
    rec[2, loo.LO_KHAT], rec[7, loo.LO_KHAT], rec[10, loo.LO_KHAT] = np.inf, 0.95, 0.6
    rec[[0, 1, 3, 4, 5, 6, 8, 9, 11], loo.LO_KHAT] *= 0.4
    res = loo.summarise(rec, S, k_lim)
    assert res['khat_threshold'] == 0.5 and res['n_bad'] == 3 and res['worst'] == (1, 3) and res['n'] == S
    np.testing.assert_allclose(res['elpd_loo'], rec[:, 3].sum())
    np.testing.assert_allclose(res['p_loo'], (rec[:, 0] - rec[:, 3]).sum())
    np.testing.assert_allclose(res['p_waic'], rec[:, 2].sum() / 99)
    np.testing.assert_allclose(res['elpd_waic'], (rec[:, 0] - rec[:, 2] / 99).sum())
    np.testing.assert_allclose(res['se_elpd_loo'], np.sqrt(12 * rec[:, 3].var(ddof=1)))
    np.testing.assert_allclose(res['site_elpd_loo'], [rec[0:4, 3].sum(), rec[4:9, 3].sum(), rec[9:12, 3].sum()])
    for name in ('elpd_loo', 'p_loo', 'elpd_waic', 'p_waic'):
        np.testing.assert_allclose(res['site_' + name].sum(), res[name], rtol=1e-13)
    assert loo.khat_threshold(4000) == 0.7 and abs(loo.khat_threshold(80) - (1 - 1 / np.log10(80))) < 1e-15


# ------------------------------------------------------------------ Master.loo on the CPU oracle engine
@pytest.mark.parametrize('J,K', [(4, 4), (5, 3)])
def test_master_loo_on_the_cpu_engine(J, K):
    D = 3
    conf = fit.configurations(J=J, D=D, K=K, npg=30, siter=40, run_ep=True, damp=0.4)
    M = fit.main('m4b', conf, ret_master=True, verbose=False, _engine_factory=factory)
    assert isinstance(M, Master) and isinstance(M.engine, OracleEngine) and not hasattr(M.engine, 'loo')
    with pytest.raises(RuntimeError, match='before at least one iteration'):
        M.loo()
    assert M.run(2, verbose=False, calc_moments=False, seed=5) == 0
    multi = not M.model_name.endswith('_sg')
    assert multi == (K < J)
    res = M.loo()
    S = res['n']
    assert S == 80 and res['lpd'].shape == (M.N,) and res['site_elpd_loo'].shape == (K,)
    mid, gauss, _ = M._site_spec()
    j_ind = np.asarray(M.A_n['j_ind']) if multi else None
    for k in range(K):
        sl = slice(M.k_lim[k], M.k_lim[k + 1])
        exp = loo.loo_host(mid, D, int(M._site_ng[k]), gauss, M.engine.get_draws(k, all_params=True), M.X[sl],
                           j_ind[sl] - 1 if multi else None, M.y[sl])
        np.testing.assert_array_equal(res['lpd'][sl], exp[:, loo.LO_LPD])
        np.testing.assert_array_equal(res['elpd_loo_i'][sl], exp[:, loo.LO_ELPD])
        np.testing.assert_array_equal(res['khat'][sl], exp[:, loo.LO_KHAT])
        np.testing.assert_array_equal(res['wess'][sl], exp[:, loo.LO_WESS])
        np.testing.assert_allclose(res['p_waic_i'][sl], exp[:, loo.LO_LL_M2] / (S - 1), rtol=1e-15)
        np.testing.assert_allclose(res['site_elpd_loo'][k], exp[:, loo.LO_ELPD].sum(), rtol=1e-13)
    assert res['elpd_loo'] < res['lpd'].sum() and res['p_loo'] > 0 and res['p_waic'] > 0
    for name in ('elpd_loo', 'p_loo', 'elpd_waic', 'p_waic'):
        np.testing.assert_allclose(res['site_' + name].sum(), res[name], rtol=1e-12)
    np.testing.assert_allclose(res['elpd_loo'] + res['p_loo'], res['lpd'].sum(), rtol=1e-12)
    assert res['n_bad'] == int(np.count_nonzero(res['khat'] > res['khat_threshold']))

    def from_cavity(data, stan_params):                  # draws of phi alone, as an injector gives them
        z = np.random.RandomState(stan_params['seed'] % 1000).randn(80, M.dphi)
        return data['mu_phi'] + np.linalg.solve(np.linalg.cholesky(data['Omega_phi']).T, z.T).T
    M._sample_injector = from_cavity
    M.run(1, verbose=False, seed=3)
    with pytest.raises(RuntimeError, match='injected'):
        M.loo()
