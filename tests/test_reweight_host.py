"""reweight.py, the NumPy statement of the reuse of tilted draws across EP iterations (include/epx.h: epx_reweight_batch),
anchored to things outside itself: NumPy's own moments, the oracle's moment stage, loo.psis_host and a Gaussian case with a
closed form.  CPU only."""

import math

import numpy as np
import pytest

from epstan_amd import loo, reweight
from oracle import ep_oracle


def _case(d, S, seed, scale):
    rng = np.random.RandomState(seed)
    A = rng.randn(d, d + 3)
    Oo = A.dot(A.T) / (d + 3) + 0.5 * np.eye(d)
    mo = 0.5 * rng.randn(d)
    B = rng.randn(d, d)
    On = Oo * (1 + scale) + scale * 0.1 * (B + B.T) / np.sqrt(d)
    mn = mo + scale * rng.randn(d)
    phi = 0.3 * mo + rng.randn(S, d).dot(np.linalg.cholesky(np.linalg.inv(Oo + 2 * np.eye(d))).T)
    Q = Oo + np.eye(d)
    r = Q.dot(0.2 * rng.randn(d))
    return phi, Oo, mo, On, mn, Q, r


@pytest.mark.parametrize('prec_estim', ['sample', 'olse'])
@pytest.mark.parametrize('d,S', [(4, 20), (4, 64), (18, 203)])
def test_identical_cavities_give_the_plain_moments(d, S, prec_estim):
    phi, Oo, mo, _, _, Q, r = _case(d, S, 7, 0.1)
    out = reweight.reweight_host(phi, Oo, mo, Oo, mo, Q, r, prec_estim)
    assert np.all(out['lr'] == 0.0)
    assert np.isposinf(out['khat'])
    np.testing.assert_allclose(out['wess'], S, rtol=1e-13)
    np.testing.assert_allclose(out['lw'], -math.log(S), rtol=1e-13)
    C = phi - phi.mean(axis=0)
    np.testing.assert_allclose(out['mean'], phi.mean(axis=0), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(out['scatter'], C.T.dot(C), rtol=1e-12, atol=1e-12)
    dQi, dri, _, _, posdef = ep_oracle.tilted_moments(phi, Q, r, prec_estim)
    assert posdef and out['ok']
    scale = np.abs(dQi).max()
    np.testing.assert_allclose(out['dQi'], dQi, rtol=1e-12, atol=1e-12 * scale)
    np.testing.assert_allclose(out['dri'], dri, rtol=1e-12, atol=1e-12 * np.abs(dri).max())


@pytest.mark.parametrize('d,S,scale', [(4, 20, 0.1), (4, 25, 0.1), (4, 64, 0.02), (18, 203, 0.1), (34, 203, 0.02)])
def test_weights_are_those_of_psis_host(d, S, scale):
    phi, Oo, mo, On, mn, Q, r = _case(d, S, 1000 * d + S, scale)
    out = reweight.reweight_host(phi, Oo, mo, On, mn, Q, r, 'sample')
    ref = loo.psis_host(-out['lr'][None])[0]
    if np.isinf(ref[1]):
        assert np.isposinf(out['khat'])
    else:
        np.testing.assert_allclose(out['khat'], ref[1], rtol=1e-13)
    assert np.isinf(ref[1]) == (S == 20)                       # M = 4: not smoothed
    np.testing.assert_allclose(out['wess'], ref[2], rtol=1e-13)
    np.testing.assert_allclose(np.exp(out['lw']).sum(), 1.0, rtol=1e-13)
    # the ratio is the difference of the two cavities' log densities up to a constant
    def logn(x, Om, mu):
        return -0.5 * np.einsum('si,ij,sj->s', x - mu, Om, x - mu)
    diff = logn(phi, On, mn) - logn(phi, Oo, mo)
    np.testing.assert_allclose(out['lr'] - out['lr'][0], diff - diff[0], rtol=0, atol=1e-10 * np.abs(diff).max())
    # the same in extended precision
    wide = reweight.reweight_host(phi.astype(np.longdouble), Oo, mo, On, mn, Q, r, 'sample')
    assert wide['mean'].dtype == np.longdouble and wide['lw'].dtype == np.longdouble
    np.testing.assert_allclose(out['mean'], wide['mean'].astype(np.float64), rtol=1e-9, atol=1e-12)


def test_analytic_gaussian_case():
    """Tilted distribution exactly Gaussian: likelihood precision L about a, cavity N(mu, Om^-1): the tilted precision
    is Om + L and its mean (Om + L)^-1 (Om mu + L a).  The draws come from the old tilted distribution; the weighted mean
    must lie within 5 standard errors (at the weighted effective sample size) of the new tilted mean, and strictly
    closer to it than the plain mean of the draws."""
    d, S = 3, 20000
    rng = np.random.RandomState(11)
    A = rng.randn(d, d + 3)
    L = A.dot(A.T) / (d + 3) + 0.5 * np.eye(d)
    a = rng.randn(d)
    Oo, mo = np.diag([1.0, 2.0, 0.7]), np.array([0.3, -0.2, 0.1])
    On, mn = Oo * 1.15 + 0.05, mo + np.array([0.25, -0.2, 0.15])
    So = np.linalg.inv(Oo + L)
    m_old = So.dot(Oo.dot(mo) + L.dot(a))
    Sn = np.linalg.inv(On + L)
    m_new = Sn.dot(On.dot(mn) + L.dot(a))
    phi = m_old + rng.randn(S, d).dot(np.linalg.cholesky(So).T)
    Q = On + L
    out = reweight.reweight_host(phi, Oo, mo, On, mn, Q, Q.dot(m_new), 'sample')
    assert np.isfinite(out['khat']) and out['khat'] < loo.khat_threshold(S)
    err = np.abs(out['mean'] - m_new)
    se = np.sqrt(np.diag(Sn) / out['wess'])
    print('khat %.3f wess/S %.3f, error / se %s' % (out['khat'], out['wess'] / S, err / se))
    assert np.all(err <= 5 * se)
    assert np.linalg.norm(out['mean'] - m_new) < np.linalg.norm(phi.mean(axis=0) - m_new)
    assert np.all(np.abs(out['mean'] - m_new) < np.abs(phi.mean(axis=0) - m_new))


def test_reuse_ok_truth_table():
    S = 1000
    thr = loo.khat_threshold(S)
    assert thr == pytest.approx(1 - 1 / 3.0)
    inf = float('inf')
    assert reweight.reuse_ok(0.3, 600.0, S) is True
    assert reweight.reuse_ok(thr, 500.0, S) is True                 # both limits are inclusive
    assert reweight.reuse_ok(np.nextafter(thr, 1.0), 600.0, S) is False
    assert reweight.reuse_ok(0.3, 499.0, S) is False
    assert reweight.reuse_ok(inf, 600.0, S) is True                 # not smoothed: the effective sample size decides
    assert reweight.reuse_ok(inf, 499.0, S) is False
    assert reweight.reuse_ok(-inf, 600.0, S, k_max=-inf) is True
    assert reweight.reuse_ok(0.0, 1000.0, S, k_max=-inf) is False
    assert reweight.reuse_ok(5.0, 1.0, S, k_max=inf, min_ess=0) is True
    assert reweight.reuse_ok(float('nan'), float('nan'), S, k_max=inf, min_ess=0) is False
    assert reweight.reuse_ok(0.69, 600.0, S, k_max=0.7) is True
    assert reweight.reuse_ok(0.69, 600.0, S, min_ess=0.7) is False
    got = reweight.reuse_ok(np.array([0.3, inf, 0.9, 0.3]), np.array([600.0, 600.0, 600.0, 100.0]), S)
    assert got.tolist() == [True, True, False, False]
    assert (reweight.RW_KHAT, reweight.RW_WESS, reweight.RW_COUNT) == (0, 1, 2)


def test_sample_estimate_refuses_a_small_effective_sample():
    """scale = 0.3 at (d, S) = (18, 64): the weighted effective sample size falls below d + 2."""
    phi, Oo, mo, On, mn, Q, r = _case(18, 64, 1000 * 18 + 64, 0.3)
    out = reweight.reweight_host(phi, Oo, mo, On, mn, Q, r, 'sample')
    assert out['wess'] - 18 - 2 <= 0
    assert not out['ok'] and not out['dQi'].any() and not out['dri'].any()
    assert np.all(np.isfinite(out['mean'])) and np.all(np.isfinite(out['scatter']))
    dQi, dri, ok = reweight.precision_host(out['mean'], out['scatter'], 20.0, Q, r, 'sample')
    assert not ok and not dQi.any()
    assert reweight.precision_host(out['mean'], out['scatter'], 20.5, Q, r, 'sample')[2]
    with pytest.raises(ValueError):
        reweight.precision_host(out['mean'], out['scatter'], 64.0, Q, r, 'mean')


def test_a_ratio_that_is_not_finite_voids_the_site():
    phi, Oo, mo, On, mn, Q, r = _case(4, 25, 3, 0.1)
    phi[7, 2] = np.nan
    out = reweight.reweight_host(phi, Oo, mo, On, mn, Q, r, 'olse')
    assert np.isnan(out['khat']) and np.isnan(out['wess']) and not out['ok']
    assert not out['dQi'].any() and not out['dri'].any()
