"""evidence.py, the NumPy statement of the bridge-sampling site normaliser (include/epx.h, epx_site_evidence) and of EP's
log evidence, on the CPU: an exact proposal, `combine` on exactly Gaussian sites, the estimate against quadrature on a
three-parameter site (m1b), the same site with Laplace latents (m5b) and in the Gaussian family (m1a), the target against
the sampler's own density for all ten models, the proposal's stream, every refusal, and `Master.log_evidence` with the
oracle standing in for the device engine.

The quadrature site: 12 rows at D = 1, one site, a diagonal cavity (precision 4 on every log scale, 1 on every location).
  m1b: theta = (log sigma_a, beta, eta), a tensor grid of 129^3 points over +-7 prior standard deviations; the grid of
       twice the step (65^3) gives the same log integral within 1e-6 (asserted).
  m1a: theta = (log sigma, log sigma_a, beta, eta).  At given scales the integrand is Gaussian in (beta, eta): that
       integral in closed form from the rows' sufficient statistics, then a tensor grid of 801^2 points over the two log
       scales (401^2 within 1e-6); the 1/2 log 2 pi per row is written out here on its own.
  m5b: six coordinates.  The likelihood depends on theta through a = mu_a + eta sigma_a and b = mu_b + etb sigma_b alone,
       which are independent under a diagonal cavity, so log Z_k = log int int p_a(a) p_b(b) lik(a, b) da db with p_a the
       density of a location (normal) plus a scale (log-normal) times a standard Laplace latent: the normal-Laplace
       convolution in closed form (erfcx), a grid over the log scale, then a tensor grid over (a, b), every grid against
       the grid of twice its step within 1e-6.  This is log Z_k against the NORMALISED cavity and prior: it checks c_lat =
       n_lat log 2 of `site_log_z`.

SIGMA, the standard deviation of LOGZ - quadrature on the m1b site over the sampler's seed (4 chains x 400 kept draws
from oracle.nuts_oracle.nuts_sites), comes from scripts/evidence_study.py over 20 seeds (1..20): sd 0.0107, mean error
-0.0023, inside 3 sd / sqrt(20) = 0.0072.  The committed tests run 3 other seeds at 6 SIGMA =
0.064.  The m1a and the m5b site are held to the SAME 0.064, the bound of the m1b study, which is tighter for them than
six of their own standard deviations: the same study gives sd 0.0162 for the m1a site and 0.0245 for the m5b site
(largest errors over the 20 seeds 0.033 and 0.047), so 0.064 is 4.0 sd for m1a and 2.6 sd for m5b.  What these two
cases are there to catch -- a missing 1/2 log 2 pi per row (12 x 0.92) or a wrong c_lat (2 log 2 against log 2 pi: 0.45)
-- is many times the bound; a failure by a few hundredths on another seed would be sampling noise, not a wrong constant."""

import math
import os
import sys

import numpy as np
import pytest
import scipy.special

import test_predict_host as tph
from epstan_amd import engine as _engine, evidence as ev, newgroup
from epstan_amd.method import Master
from oracle import nuts_oracle as no

LD = np.longdouble
SIGMA = 0.0107                                           # scripts/evidence_study.py, 20 seeds (see above)
MODELS = ['m1b_sg', 'm2b_sg', 'm3b_sg', 'm4b_sg', 'm5b_sg', 'm1a_sg', 'm2a_sg', 'm3a_sg', 'm4a_sg', 'm5a_sg']


def _spec(model):
    return no.MODEL_IDS[model] % 5, no.is_gauss(model)


# ------------------------------------------------------------------ 1. an exact proposal
def test_exact_proposal_gives_log_c_in_two_iterations():
    """m1b at D = 1 without rows: lq = -1/2 (phi - mu)' Omega (phi - mu) - 1/2 eta^2, an unnormalised Gaussian in P = 3
    with log c = 3/2 log 2 pi - 1/2 log det Omega.  With the true (m, L) as the proposal every term is log c."""
    rng = np.random.RandomState(1)
    A = rng.randn(2, 4)
    Om = A.dot(A.T) / 4 + 0.5 * np.eye(2)
    mu = np.array([0.3, -0.7])
    cov = np.zeros((3, 3))
    cov[:2, :2] = np.linalg.inv(Om)
    cov[2, 2] = 1.0
    m, L = np.concatenate((mu, [0.0])), np.linalg.cholesky(cov)
    theta = m + rng.randn(4 * 50, 3).dot(L.T)
    log_c = 1.5 * math.log(2 * math.pi) - 0.5 * np.linalg.slogdet(Om)[1]
    rec, terms = ev.site_evidence_host(0, 1, False, np.zeros((0, 1)), np.zeros(0), None, mu, Om, theta, 4, 11, 5,
                                       proposal=(m, L))
    np.testing.assert_allclose(terms['l1'], log_c, rtol=0, atol=1e-12)
    np.testing.assert_allclose(terms['l2'], log_c, rtol=0, atol=1e-12)
    assert abs(rec[ev.EV_LOGZ] - log_c) <= 1e-12 and abs(rec[ev.EV_LOGZ_IS] - log_c) <= 1e-12
    assert rec[ev.EV_ITERS] <= 2 and rec[ev.EV_N1] == 100
    assert rec[ev.EV_RE2] <= 1e-20


# ------------------------------------------------------------------ 2. combine on exactly Gaussian sites
def test_combine_on_gaussian_sites_is_the_exact_evidence():
    rng = np.random.RandomState(2)
    d, K = 4, 3
    B = rng.randn(d, d + 2)
    Q0, r0 = B.dot(B.T) / d + np.eye(d), rng.randn(d)
    Qi, ri, c = np.zeros((d, d, K)), np.zeros((d, K)), rng.randn(K)
    for k in range(K):
        B = rng.randn(d, d)
        Qi[:, :, k], ri[:, k] = B.dot(B.T) / d, rng.randn(d)
    Q, r = Q0 + Qi.sum(axis=2), r0 + ri.sum(axis=1)
    # the analytic log Z_k of t_k = exp(-1/2 x' A x + b' x + c) against its normalised cavity
    log_zk = [c[k] + ev.log_partition(Q, r) - ev.log_partition(Q - Qi[:, :, k], r - ri[:, k]) for k in range(K)]
    exact = ev.log_partition(Q, r) - ev.log_partition(Q0, r0) + c.sum()
    assert abs(ev.combine(Q, r, Q0, r0, Qi, ri, log_zk) - exact) <= 1e-10
    # Phi against a one-dimensional integral
    assert abs(ev.log_partition([[2.0]], [0.6]) - math.log(math.sqrt(2 * math.pi / 2.0) * math.exp(0.09))) <= 1e-14


# ------------------------------------------------------------------ 3. quadrature truth
QUAD_N = 12


def quad_site(model, k=0):
    """(X (12, 1), y, mu, Omega) of quadrature site k: the rows from a fixed seed, a diagonal cavity."""
    rng = np.random.RandomState(70 + k)
    X = rng.randn(QUAD_N, 1) * 1.3
    if no.is_gauss(model):
        y = 0.3 + 0.8 * X[:, 0] + 0.7 * rng.randn(QUAD_N)
    else:
        y = (rng.rand(QUAD_N) < 1 / (1 + np.exp(-(0.4 + 0.9 * X[:, 0])))).astype(np.float64)
    mid, gauss = _spec(model)
    loc, ls = (1.0, 0.2), (4.0, -0.3)                    # (precision, mean) of a location and of a log scale
    kinds = {0: [ls, loc], 4: [loc, ls, loc, ls]}[mid]
    if gauss:
        kinds = [ls] + kinds
    return X, y, np.array([m for _, m in kinds]), np.diag([p for p, _ in kinds])


def _grid_lse(f, axes):
    """log of the rectangle-rule integral of exp(f) over the tensor grid `axes`, f evaluated slab by slab of the first."""
    vol = np.prod([a[1] - a[0] for a in axes])
    rest = np.meshgrid(*axes[1:], indexing='ij')
    parts = np.array([_lse(f(x0, *rest)) for x0 in axes[0]])
    return _lse(parts) + math.log(vol)


def _lse(v):
    top = np.max(v)
    return top + math.log(np.sum(np.exp(v - top)))


def _axes(centres, halfwidths, n):
    return [np.linspace(c - h, c + h, n) for c, h in zip(centres, halfwidths)]


def _bern_ll(y, f):
    return y * f - (np.maximum(f, 0) + np.log1p(np.exp(-np.abs(f))))


_TRUTH = {}


def quad_truth(model, k=0):
    """(log int exp(lq), log Z_k against the normalised cavity and prior) of quadrature site k; either may be None
    where the route does not give it.  Every grid is compared with the grid of twice its step."""
    if (model, k) in _TRUTH:
        return _TRUTH[(model, k)]
    X, y, mu, Om = quad_site(model, k)
    x, prec = X[:, 0], np.diag(Om)
    mid, gauss = _spec(model)
    if model == 'm1b_sg':
        def lq(lsa, beta, eta):
            out = -0.5 * prec[0] * (lsa - mu[0]) ** 2 - 0.5 * prec[1] * (beta - mu[1]) ** 2 - 0.5 * eta ** 2
            a = eta * np.exp(lsa)
            for i in range(QUAD_N):
                out = out + _bern_ll(y[i], a + beta * x[i])
            return out
        val = [_grid_lse(lq, _axes([mu[0], mu[1], 0.0], [3.5, 7.0, 7.0], n)) for n in (129, 65)]
        res = (val[0], val[0] + 0.5 * np.log(prec).sum() - 1.5 * math.log(2 * math.pi))
    elif model == 'm1a_sg':
        n, sy, sx, syy, sxy, sxx = QUAD_N, y.sum(), x.sum(), y.dot(y), x.dot(y), x.dot(x)

        def lq(ls, lsa):
            """log of the integral over (beta, eta), a Gaussian one at given scales: -1/2 v' H v + g' v + c0."""
            w, s = np.exp(-2 * ls), np.exp(lsa)
            h11, h12, h22 = prec[2] + w * sxx, w * s * sx, 1 + w * n * s * s
            g1, g2 = prec[2] * mu[2] + w * sxy, w * s * sy
            det = h11 * h22 - h12 * h12
            quad = (h22 * g1 * g1 - 2 * h12 * g1 * g2 + h11 * g2 * g2) / det
            return (-0.5 * prec[0] * (ls - mu[0]) ** 2 - 0.5 * prec[1] * (lsa - mu[1]) ** 2
                    - n * 0.5 * math.log(2 * math.pi) - n * ls - 0.5 * prec[2] * mu[2] ** 2 - 0.5 * w * syy
                    + 0.5 * quad + math.log(2 * math.pi) - 0.5 * np.log(det))
        val = [_grid_lse(lq, _axes([mu[0], mu[1]], [4.0, 4.0], n_)) for n_ in (801, 401)]
        res = (val[0], val[0] + 0.5 * np.log(prec).sum() - 2.0 * math.log(2 * math.pi))
    else:
        assert model == 'm5b_sg'

        def coef_logpdf(v, loc_m, loc_p, ls_m, ls_p, n):
            """log density at v of loc + e^ls z: loc ~ N(loc_m, 1 / loc_p), ls ~ N(ls_m, 1 / ls_p), z standard Laplace."""
            sg = 1 / math.sqrt(loc_p)
            ls = np.linspace(ls_m - 8 / math.sqrt(ls_p), ls_m + 8 / math.sqrt(ls_p), n)[:, None]
            b, t = np.exp(ls), (v - loc_m)[None, :]
            z1, z2 = (sg * sg / b - t) / (sg * math.sqrt(2)), (sg * sg / b + t) / (sg * math.sqrt(2))
            conv = np.exp(-0.5 * (t / sg) ** 2) * (scipy.special.erfcx(z1) + scipy.special.erfcx(z2)) / (4 * b)
            w = np.exp(-0.5 * ls_p * (ls - ls_m) ** 2) * math.sqrt(ls_p / (2 * math.pi)) * (ls[1, 0] - ls[0, 0])
            return np.log((w * conv).sum(axis=0))

        def log_zk(n, n_ls):
            a = np.linspace(mu[0] - 12, mu[0] + 12, n)
            b = np.linspace(mu[2] - 12, mu[2] + 12, n)
            out = coef_logpdf(a, mu[0], prec[0], mu[1], prec[1], n_ls)[:, None] \
                + coef_logpdf(b, mu[2], prec[2], mu[3], prec[3], n_ls)[None, :]
            for i in range(QUAD_N):
                out = out + _bern_ll(y[i], a[:, None] + b[None, :] * x[i])
            return _lse(out) + math.log((a[1] - a[0]) * (b[1] - b[0]))
        val = [log_zk(801, 401), log_zk(401, 401), log_zk(801, 201)]
        res = (None, val[0])
    assert max(abs(v - val[0]) for v in val[1:]) < 1e-6, val
    _TRUTH[(model, k)] = res
    return res


def quad_draws(model, seed, k=0, chains=4, keep=400):
    """The oracle sampler's draws (chains x keep, P) of quadrature site k, chain-major."""
    X, y, mu, Om = quad_site(model, k)
    draws = no.nuts_sites(model, X, y, [0, QUAD_N], mu[None], Om[None], [seed], chains=chains, iter=2 * keep)[0]
    return draws[0].reshape(chains * keep, -1)


def quad_estimate(model, seed, k=0):
    """(the record, log Z_k by site_log_z) of quadrature site k from the oracle sampler's draws under `seed`."""
    mid, gauss = _spec(model)
    X, y, mu, Om = quad_site(model, k)
    rec = ev.site_evidence_host(mid, 1, gauss, X, y, None, mu, Om, quad_draws(model, seed, k), 4, seed, k)[0]
    return rec, ev.site_log_z(rec[ev.EV_LOGZ], Om, ev.n_latents(mid, 1), mid)


@pytest.mark.parametrize('model', ['m1b_sg', 'm1a_sg', 'm5b_sg'])
def test_estimate_against_quadrature(model):
    logq, logzk = quad_truth(model)
    for seed in (101, 102, 103):
        rec, zk = quad_estimate(model, seed)
        print('%s seed %d: LOGZ %.5f, log Z_k %.5f (quadrature %s, %.5f), iters %d, re2 %.2e, khat %.3f'
              % (model, seed, rec[ev.EV_LOGZ], zk, logq, logzk, rec[ev.EV_ITERS], rec[ev.EV_RE2], rec[ev.EV_KHAT]))
        assert rec[ev.EV_ITERS] <= ev.MAX_ITERS and np.isfinite(rec).all()
        if logq is not None:
            assert abs(rec[ev.EV_LOGZ] - logq) <= 6 * SIGMA
        assert abs(zk - logzk) <= 6 * SIGMA
        assert abs(rec[ev.EV_LOGZ_IS] - rec[ev.EV_LOGZ]) <= 0.5        # the plain importance estimate, far coarser


# ------------------------------------------------------------------ 4. lq against the sampler's own density
@pytest.mark.parametrize('model', MODELS)
@pytest.mark.parametrize('D,ngs', [(1, None), (3, None), (2, (4, 1, 6))])
def test_target_is_the_samplers_density(model, D, ngs):
    """lq = the oracle's lp for the logistic family, lp - n 1/2 log 2 pi for the Gaussian one (the sampler drops it)."""
    mid, gauss = _spec(model)
    multi = ngs is not None
    name = model[:-3] if multi else model
    ng = len(ngs) if multi else 1
    n = int(np.sum(ngs)) if multi else 9
    rng = np.random.RandomState(5 + D)
    X = rng.randn(n, D)
    y = 0.3 + rng.randn(n) if gauss else (rng.rand(n) < 0.5).astype(np.float64)
    d, P = ev.site_dims(mid, D, gauss, ng)
    assert (d, P) == no.dims(name, D, ng)
    A = rng.randn(d, d + 2)
    Om, mu = A.dot(A.T) / d + 0.3 * np.eye(d), 0.3 * rng.randn(d)
    theta = 0.6 * rng.randn(7, P)
    groups = np.repeat(np.arange(ng), ngs) if multi else None
    gl = np.concatenate(([0], np.cumsum(ngs))) if multi else None
    lq = ev.log_target(mid, D, gauss, X, y, groups, mu, Om, theta)
    lp = np.array([no.logdensity_grad(name, X, y, mu, Om, th, gl)[0] for th in theta])
    const = -0.5 * n * math.log(2 * math.pi) if gauss else 0.0
    np.testing.assert_allclose(lq, lp + const, rtol=1e-12, atol=1e-12)
    wide = ev.log_target(mid, D, gauss, X, y, groups, mu, Om, theta.astype(LD))
    assert wide.dtype == LD
    np.testing.assert_allclose(lq, wide.astype(np.float64), rtol=1e-13, atol=1e-13)


# ------------------------------------------------------------------ 5. the stream
def test_proposal_stream_depends_on_seed_label_draw_and_element_only():
    seed, label = 2 ** 40 + 3, 77
    z = ev.proposal_normals(seed, label, 9, 7)
    assert z.shape == (9, 7) and np.isfinite(z).all()
    # one element at a time, straight from the counter (r, K_BRIDGE, e >> 1, 0)
    for r, e in ((0, 0), (3, 4), (8, 5), (8, 6)):
        u1, u2 = newgroup.rng_u2(newgroup.make_key(seed, label), r, 8, e >> 1, 0)
        rad, ang = math.sqrt(-2 * math.log(float(u1))), 6.283185307179586476925286766559 * float(u2)
        assert abs(z[r, e] - (rad * math.sin(ang) if e & 1 else rad * math.cos(ang))) <= 4e-16 * (1 + abs(z[r, e]))
    # more draws or more coordinates do not move the others; another seed or label moves all
    big = ev.proposal_normals(seed, label, 20, 12)
    assert big[:9, :7].tobytes() == z.tobytes()
    assert np.all(ev.proposal_normals(seed + 1, label, 9, 7) != z) and np.all(ev.proposal_normals(seed, label + 1, 9, 7) != z)
    assert ev.K_BRIDGE == 8 and ev.K_BRIDGE not in (newgroup.K_NEWGROUP, 7)
    # the proposal draws of a site are m + L z of that stream
    X, y, mu, Om = quad_site('m1b_sg')
    theta = quad_draws('m1b_sg', 9, keep=40)
    t = ev.site_evidence_host(0, 1, False, X, y, None, mu, Om, theta, 4, seed, label)[1]
    np.testing.assert_allclose(t['prop'], t['m'] + ev.proposal_normals(seed, label, 80, 3).dot(t['L'].T), rtol=1e-15)
    m, L = ev.fit_proposal(theta[ev.split(160, 4)[0]])
    assert np.array_equal(ev.split(8, 2)[0], [0, 1, 4, 5]) and np.array_equal(ev.split(10, 2)[1], [2, 3, 4, 7, 8, 9])
    np.testing.assert_allclose(L.dot(L.T), np.cov(theta[ev.split(160, 4)[0]].T), rtol=1e-10)
    np.testing.assert_array_equal(t['m'], m)


# ------------------------------------------------------------------ 6. refusals and soft failures
def _refused(match, S=160, chains=4, D=1, mid=0, P=None, theta=None):
    d, Pm = ev.site_dims(mid, D, False)
    theta = np.zeros((S, Pm if P is None else P)) if theta is None else theta
    with pytest.raises(ValueError, match=match):
        ev.site_evidence_host(mid, D, False, np.zeros((0, D)), np.zeros(0), None, np.zeros(d), np.eye(d), theta, chains, 0, 0)


def test_fit_set_smaller_than_2p_is_refused():
    _refused(r'fit set holds 4 draws \(the first 1 of each of 4 chains\), the proposal of P = 3 coordinates needs at least 6',
             S=8)
    ev.check_sizes(16, 4, 3, 1)                          # n = 4: |F| = 8 >= 6
    with pytest.raises(ValueError, match='fit set holds 4 draws'):
        ev.check_sizes(12, 4, 3, 1)                      # n = 3: the first 1 of each chain


def test_chains_that_do_not_divide_s_are_refused():
    _refused('S = 161 draws are no multiple of chains = 4', S=161)


def test_more_than_128_columns_are_refused():
    with pytest.raises(ValueError, match='D = 129 columns, at most 128'):
        ev.check_sizes(4000, 4, 131, 129)


def test_a_p_beyond_the_lds_limit_is_refused():
    assert ev.max_coords(32) == 166 and ev.max_coords(32) >= ev.site_dims(3, 32, False)[1] == 99
    assert ev.site_dims(3, 128, False)[1] > ev.max_coords(128)          # C5's m4b at D = 128: out of scope
    with pytest.raises(ValueError, match='P = 167 sampled coordinates, at most 166 at D = 32'):
        ev.check_sizes(4000, 4, 167, 32)
    ev.check_sizes(4000, 4, 166, 32)


def test_soft_failures_are_nan_records():
    X, y, mu, Om = quad_site('m1b_sg')
    theta = quad_draws('m1b_sg', 9, keep=40)
    bad = theta.copy()
    bad[150, 1] = np.nan                                 # in E: a non-finite l1
    rec = ev.site_evidence_host(0, 1, False, X, y, None, mu, Om, bad, 4, 0, 0)[0]
    assert np.isnan(rec[[ev.EV_LOGZ, ev.EV_LOGZ_IS, ev.EV_RE2, ev.EV_KHAT]]).all()
    assert rec[ev.EV_ITERS] == 0 and rec[ev.EV_N1] == 80
    bad = theta.copy()
    bad[3, 0] = np.inf                                   # in F: no factor
    rec, t = ev.site_evidence_host(0, 1, False, X, y, None, mu, Om, bad, 4, 0, 0)
    assert np.isnan(rec[ev.EV_LOGZ]) and t['L'] is None
    dup = theta.copy()
    dup[:, 2] = dup[:, 1]                                # a duplicated coordinate: singular C
    rec = ev.site_evidence_host(0, 1, False, X, y, None, mu, Om, dup, 4, 0, 0)[0]
    assert np.isnan(rec[ev.EV_LOGZ]) and rec[ev.EV_ITERS] == 0


# ------------------------------------------------------------------ Master.log_evidence, the oracle as the engine
def quad_master(model='m1b_sg', K=2, **kw):
    """A Master over K quadrature sites (one group each), 4 chains x 400 kept draws."""
    sites = [quad_site(model, k) for k in range(K)]
    X, y = np.concatenate([s[0] for s in sites]), np.concatenate([s[1] for s in sites])
    d = sites[0][2].shape[0]
    kw.setdefault('_engine_factory', tph.factory)
    return Master(model, X, y if no.is_gauss(model) else y.astype(int), site_sizes=[QUAD_N] * K,
                  prior={'Q': np.diag(np.diag(sites[0][3])), 'r': np.zeros(d)}, chains=4, iter=800, df0=0.5, **kw)


def master_truth(M):
    """log Z_EP of the Master's current approximation with every log Z_k from quadrature at the current cavities (m1b,
    D = 1: a tensor grid as quad_truth's, here with the full cavity precision)."""
    log_zk = []
    for k in range(M.K):
        Om, mu = M.engine.get_cavity(k)
        sl = slice(int(M.k_lim[k]), int(M.k_lim[k + 1]))
        x, y = M.X[sl, 0], M.y[sl].astype(np.float64)

        def lq(lsa, beta, eta):
            u, v = lsa - mu[0], beta - mu[1]
            out = -0.5 * (Om[0, 0] * u * u + 2 * Om[0, 1] * u * v + Om[1, 1] * v * v) - 0.5 * eta ** 2
            a = eta * np.exp(lsa)
            for i in range(x.shape[0]):
                out = out + _bern_ll(y[i], a + beta * x[i])
            return out
        sd = np.sqrt(np.diag(np.linalg.inv(Om)))
        val = [_grid_lse(lq, _axes([mu[0], mu[1], 0.0], [7 * sd[0], 7 * sd[1], 7.0], n)) for n in (129, 65)]
        assert abs(val[0] - val[1]) < 1e-6
        log_zk.append(ev.site_log_z(val[0], Om, 1, 0))
    return ev.combine(M.Q, M.r, M.Q0, M.r0, M.Qi, M.ri, log_zk), np.array(log_zk)


def test_master_log_evidence_refusals_and_value():
    M = quad_master()
    with pytest.raises(RuntimeError, match='before at least one iteration'):
        M.log_evidence()
    assert M.run(3, verbose=False, seed=4, calc_moments=False) == 0
    M._sample_injector = lambda data, params: np.zeros((8, 2))
    with pytest.raises(RuntimeError, match='injector'):
        M.log_evidence()
    M._sample_injector = None
    M.workers[1].phase = 0
    with pytest.raises(RuntimeError, match='Worker 1 is in phase 0'):
        M.log_evidence()
    M.workers[1].phase = 1
    before = (M.iter, M.dQi.copy(), M.dri.copy(), [M.engine.get_tilted(k) for k in range(2)],
              [M.engine.get_site(_engine.DQI, k) for k in range(2)])
    res = M.log_evidence(seed=5)
    exact, log_zk = master_truth(M)
    print('log_evidence %.5f, quadrature %.5f; site_log_z %s, quadrature %s; re2 %s, khat %s, iters %s'
          % (res['log_evidence'], exact, res['site_log_z'], log_zk, res['re2'], res['khat'], res['iters']))
    assert abs(res['log_evidence'] - exact) <= 6 * SIGMA * math.sqrt(2)
    assert np.all(np.abs(res['site_log_z'] - log_zk) <= 6 * SIGMA)
    assert res['n_bad'] == 0 and res['iters'].shape == (2,) and np.all(res['iters'] <= 1000) and np.all(res['re2'] > 0)
    assert M.iter == before[0] and np.array_equal(M.dQi, before[1]) and np.array_equal(M.dri, before[2])
    for k in range(2):
        for a, b in zip(before[3][k] + before[4][k], M.engine.get_tilted(k) + M.engine.get_site(_engine.DQI, k)):
            assert np.array_equal(np.asarray(a), np.asarray(b))
    assert M.engine.num_draws() == 1600


def test_master_refuses_too_few_draws_with_the_iterations_needed():
    M = quad_master(K=2)
    M.iter = 1                                           # (as after an iteration: the size check comes before any launch)
    for w in M.workers:
        w.stan_params['iter'] = 4                        # 2 kept draws per chain: |F| = 4 x 1
    with pytest.raises(ValueError, match=r'holds 4 draws, the proposal of P = 3 sampled coordinates needs 6: sample at '
                                         r'least 4 kept iterations per chain \(iter - warmup >= 4 at thin = 1\)'):
        M.log_evidence()


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (tph.ROOT, os.path.join(tph.ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as tdist
    from epstan_amd import dist
    import test_evidence_host as me
    tdist.init_process_group('gloo', rank=rank, world_size=world)
    M = me.quad_master(K=3, comm=dist.TorchComm())
    M.run(1, verbose=False, seed=3, calc_moments=False)
    res = M.log_evidence(seed=6)
    np.savez(os.path.join(outdir, 'r%d.npz' % rank), **dict((k, np.asarray(v)) for k, v in res.items() if k != 'ms'))
    tdist.barrier()
    tdist.destroy_process_group()


def test_two_ranks_return_what_one_rank_returns(tmp_path):
    """Three sites sharded 1 + 2: the first iteration and the evidence launch sample the same draws either way, the
    proposal's stream is keyed by the site's index among all sites, and the records are gathered: both ranks return the
    one-rank dict."""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, tph._free_port(), str(tmp_path)), nprocs=2, join=True)
    M = quad_master(K=3)
    M.run(1, verbose=False, seed=3, calc_moments=False)
    res = M.log_evidence(seed=6)
    assert res['n_bad'] == 0 and res['site_log_z'].shape == (3,)
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), 'r%d.npz' % r))
        for key in ('log_evidence', 'site_log_z', 're2', 'khat', 'iters', 'n_bad'):
            np.testing.assert_allclose(z[key], res[key], rtol=1e-10, err_msg=key)


if __name__ == '__main__':
    sys.exit(pytest.main([os.path.abspath(__file__), '-q', '-s']))
