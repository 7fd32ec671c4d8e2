"""k_ev_fit / k_ev_terms / k_ev_bridge / epx_site_evidence / Master.log_evidence on the device: the bridge-sampling site
normaliser from draws in device memory, against evidence.site_evidence_host (NumPy) on the same inputs.  Need a real
MI355X.

Injected draws.  theta = c + s z, z standard normal, the scales s between 0.02 and 0.03: draws of no tilted distribution,
but a cloud so tight that lq varies by a few units over it, and the proposal is fitted to its first halves: l1 and l2 are
the same function lq - lg at two samples of about the same distribution and the bridge converges in a few iterations.
The covariance C of the fit set has a condition number below 100, asserted: the factor and the forward substitution
then lose at most two digits.

Tolerance (derived, not tuned): the host statement is evaluated in float64 and in np.longdouble on the same inputs; on
l1, l2, LOGZ and RE2 the device may differ from the float64 host by 16 x their largest difference over the case, floored
at 1e-10 (absolute).  ITERS equal; KHAT finite in the same sites.
Measured on an MI355X over all 41 parity cases (every case prints its figures): the largest float64 - longdouble
difference of the host statements is 3.1e-12 on l1 and l2 (values of a few thousand: the Gaussian family at D = 32),
3.6e-11 on LOGZ, 9.4e-13 on LOGZ_IS and 3.3e-16 on RE2; the largest |device - host| is 2.7e-12 on l1 and l2, 9.1e-13 on
LOGZ, 4.5e-13 on LOGZ_IS and 1.1e-16 on RE2: at most 0.027 of the tolerance, the absolute floor included.  ITERS equal in
every case, 1001 included (the Gaussian family at D = 32, where the tight cloud lies far from the target); the proposal
draws lie within 1.5e-2 of their bound."""

import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from epstan_amd import engine as _engine, evidence as ev                     # noqa: E402
from epstan_amd.engine import HipEngine, MODEL_IDS, is_gauss    # noqa: E402
from test_gpu_parity import _site_problem, _engine_with_cavity, _group_problem, _group_engine     # noqa: E402
import test_evidence_host as teh                                 # noqa: E402

LD = np.longdouble
MODELS = ['m1b_sg', 'm2b_sg', 'm3b_sg', 'm4b_sg', 'm5b_sg', 'm1a_sg', 'm2a_sg', 'm3a_sg', 'm4a_sg', 'm5a_sg']
COLS = [ev.EV_LOGZ, ev.EV_LOGZ_IS, ev.EV_RE2]


def _spec(model):
    return MODEL_IDS[model] % 5, is_gauss(model)


def _draws(rng, count, chains, n, P, Pk=None):
    """(count, chains n, P) injected draws, zeros behind a site's own Pk coordinates; cond(C) of every fit set <= 100."""
    Pk = [P] * count if Pk is None else Pk
    theta = np.zeros((count, chains * n, P))
    for j in range(count):
        theta[j, :, :Pk[j]] = 0.3 * rng.randn(Pk[j]) + (0.02 + 0.01 * rng.rand(Pk[j])) * rng.randn(chains * n, Pk[j])
        F = ev.split(chains * n, chains)[0]
        cond = np.linalg.cond(np.cov(theta[j, F, :Pk[j]].T).reshape(Pk[j], Pk[j]))
        assert cond <= 100, cond
    return theta


def _host(model, D, X, y, groups, mu, Om, theta, chains, seed, label):
    """The float64 and the longdouble host statements of one site."""
    mid, gauss = _spec(model)
    with np.errstate(all='ignore'):
        return (ev.site_evidence_host(mid, D, gauss, X, y, groups, mu, Om, theta, chains, seed, label),
                ev.site_evidence_host(mid, D, gauss, X, y, groups, mu, Om, theta.astype(LD), chains, seed, label))


def _tol(a, wide):
    """16 x the largest float64 - longdouble difference, floored at 1e-10."""
    a = np.asarray(a, dtype=np.float64)
    diff = float(np.max(np.abs((a - np.asarray(wide)).astype(np.float64))))
    return max(16 * diff, 1e-10), diff


def _compare(tag, out, terms, host, wide):
    """One site's device record and terms against the host's."""
    (rec, t), (wrec, wt) = host, wide
    worst = []
    for name in ('l1', 'l2'):
        tol, diff = _tol(t[name], wt[name])
        err = np.abs(terms[name] - t[name])
        worst.append((name, float(err.max()), diff))
        assert np.all(err <= tol), (tag, name, float(err.max()), tol)
    for col in COLS:
        tol, diff = _tol(rec[col], wrec[col])
        err = abs(out[col] - rec[col])
        worst.append((col, float(err), diff))
        assert err <= tol, (tag, col, err, tol)
    print('%s: |device - host| (float64 - longdouble): %s; iters %d, khat %.3f'
          % (tag, ', '.join('%s %.1e (%.1e)' % w for w in worst), out[ev.EV_ITERS], out[ev.EV_KHAT]))
    assert out[ev.EV_ITERS] == rec[ev.EV_ITERS] and out[ev.EV_N1] == rec[ev.EV_N1]
    assert np.isfinite(out[ev.EV_KHAT]) == np.isfinite(rec[ev.EV_KHAT])
    if np.isfinite(rec[ev.EV_KHAT]):
        assert abs(out[ev.EV_KHAT] - rec[ev.EV_KHAT]) <= 1e-6 * max(1.0, abs(rec[ev.EV_KHAT]))
    np.testing.assert_allclose(terms['m'][:t['m'].shape[0]], t['m'], rtol=1e-12, atol=1e-13)
    Pk = t['L'].shape[0]
    np.testing.assert_allclose(terms['L'][:Pk, :Pk], t['L'], rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------ 1. parity with the host statement
# (D, rows, chains, n): N1 = 52, 64 and 324 = 20 slabs and a quarter; rows 1, 17 and 65 (past EPX_PR_WG_ROWS) for all ten
# models, 15 and 16 for two; P = 3 .. 100, most of them no multiple of 4 (m1b: D + 2 = 3, 7, 34).  The last two shapes:
# |F| = 3 x 25 = 75 and 2 x 27 = 54, no multiples of the four draws of a step of k_ev_fit's scatter (N1 = 75 and 54)
SHAPES = [(1, 1, 4, 26), (5, 17, 4, 32), (32, 65, 4, 162)]
CASES = [(m,) + s for m in MODELS for s in SHAPES] + [(m,) + s for m in ('m4b_sg', 'm1a_sg')
                                                      for s in ((5, 15, 4, 26), (5, 16, 2, 64), (5, 17, 3, 50), (5, 17, 2, 54))]


@pytest.mark.parametrize('model,D,rows,chains,n', CASES)
def test_injected_draws_match_the_host_statement(model, D, rows, chains, n):
    X, y, k_lim, Oms, mus, d, P = _site_problem(model, D, rows, 300 + D, K=2)
    eng, Om_dev, mu_dev = _engine_with_cavity(model, X, y, k_lim, Oms, mus)
    theta = _draws(np.random.RandomState(D + rows), 2, chains, n, P)
    seed, site0 = 2 ** 33 + 5, 7
    out, terms, ms = eng.site_evidence(seed=seed, site0=site0, theta=theta, chains=chains, with_terms=True)
    assert out.shape == (2, ev.EV_COUNT) and ms > 0
    for k in range(2):
        sl = slice(int(k_lim[k]), int(k_lim[k + 1]))
        host, wide = _host(model, D, X[sl], y[sl], None, mu_dev[k], Om_dev[k], theta[k], chains, seed, site0 + k)
        _compare('%s D=%d rows=%d N1=%d site %d' % (model, D, rows, out[k, ev.EV_N1], k), out[k], terms[k], host, wide)


@pytest.mark.parametrize('model', ['m4b', 'm1b', 'm5a'])
def test_a_three_group_site_takes_each_rows_group(model):
    D, groups = 5, [[5, 1, 9], [4, 4]]
    X, y, k_lim, g_cnt, g_lim, Oms, mus, d = _group_problem(model, D, groups, 17)
    eng, Om_dev, mu_dev = _group_engine(model, X, y, k_lim, g_cnt, g_lim, Oms, mus)
    mid, gauss = _spec(model + '_sg')
    Pk = [ev.site_dims(mid, D, gauss, len(g))[1] for g in groups]
    assert eng.P == max(Pk) and Pk[0] != Pk[1]
    theta = _draws(np.random.RandomState(3), 2, 4, 40, eng.P, Pk)
    out, terms, _ = eng.site_evidence(seed=9, site0=0, theta=theta, chains=4, with_terms=True)
    for k in range(2):
        sl = slice(int(k_lim[k]), int(k_lim[k + 1]))
        grp = np.repeat(np.arange(len(groups[k])), groups[k])
        host, wide = _host(model + '_sg', D, X[sl], y[sl], grp, mu_dev[k], Om_dev[k], theta[k, :, :Pk[k]], 4, 9, k)
        _compare('%s groups %s' % (model, groups[k]), out[k], terms[k], host, wide)
        assert np.all(terms[k]['prop'][:, Pk[k]:] == 0) and np.all(terms[k]['m'][Pk[k]:] == 0)


# ------------------------------------------------------------------ 2. independence
def _flat(out, terms):
    return out.tobytes() + b''.join(t[key].tobytes() for t in terms for key in ('l1', 'l2', 'm', 'L', 'prop'))


def test_a_sites_record_does_not_depend_on_the_call():
    model, D, rows, K = 'm4b_sg', 5, 17, 4
    X, y, k_lim, Oms, mus, d, P = _site_problem(model, D, rows, 41, K=K)
    eng, Om_dev, mu_dev = _engine_with_cavity(model, X, y, k_lim, Oms, mus)
    theta = _draws(np.random.RandomState(8), K, 4, 32, P)
    kw = dict(seed=21, chains=4, with_terms=True)
    out, terms, _ = eng.site_evidence(site0=0, theta=theta, **kw)
    again = eng.site_evidence(site0=0, theta=theta, **kw)
    assert _flat(out, terms) == _flat(again[0], again[1])
    alone = eng.site_evidence(site0=0, k0=2, count=1, theta=theta[2:3], **kw)
    assert _flat(out[2:3], terms[2:3]) == _flat(alone[0], alone[1])
    part = eng.site_evidence(site0=0, k0=1, count=3, theta=theta[1:], **kw)
    assert _flat(out[1:], terms[1:]) == _flat(part[0], part[1])
    # a context that holds the sites [2, 4) only, as another rank would: site0 = 2
    lo = int(k_lim[2])
    eng2, Om2, mu2 = _engine_with_cavity(model, X[lo:], y[lo:], k_lim[2:] - lo, Oms[2:], mus[2:])
    assert Om2.tobytes() == Om_dev[2:].tobytes() and mu2.tobytes() == mu_dev[2:].tobytes()
    shard = eng2.site_evidence(site0=2, theta=theta[2:], **kw)
    assert _flat(out[2:], terms[2:]) == _flat(shard[0], shard[1])
    moved = eng2.site_evidence(site0=3, theta=theta[2:], **kw)          # another label: another proposal sample
    assert np.all(moved[0][:, ev.EV_LOGZ] != out[2:, ev.EV_LOGZ])
    assert moved[1][0]['l1'].tobytes() == terms[2]['l1'].tobytes()       # (the tilted side does not see the stream)


# ------------------------------------------------------------------ 3. the stream
@pytest.mark.parametrize('model,D', [('m1b_sg', 1), ('m4b_sg', 5), ('m4a_sg', 32)])
def test_proposal_draws_are_m_plus_l_z_of_the_twin(model, D):
    """z of the twin is pinned as test_gpu_newgroup.py pins its latents, 1e-13 (1 + |z|); through m + L z that is
    sum_j |L_ij| 1e-13 (1 + |z_j|), plus the rounding of the sum of P + 1 terms."""
    X, y, k_lim, Oms, mus, d, P = _site_problem(model, D, 3, 5, K=2)
    eng, _, _ = _engine_with_cavity(model, X, y, k_lim, Oms, mus)
    n = 2 * -(-33 * P // 40) + 1                          # |F| >= 3.3 P draws, an odd n
    theta = _draws(np.random.RandomState(2), 2, 4, n, P)
    seed, site0 = 2 ** 45 + 17, 2 ** 31 - 3             # the last labels below 2^31
    with pytest.raises(RuntimeError, match=re.escape('outside [0,2^31)')):
        eng.site_evidence(seed=seed, site0=site0 + 1, theta=theta, chains=4)
    out, terms, _ = eng.site_evidence(seed=seed, site0=site0, theta=theta, chains=4, with_terms=True)
    for k in range(2):
        t = terms[k]
        z = ev.proposal_normals(seed, site0 + k, t['prop'].shape[0], P)
        exp = t['m'] + z.dot(t['L'].T)
        bound = (1e-13 * (1 + np.abs(z))).dot(np.abs(t['L']).T) \
            + (P + 1) * 2.0 ** -52 * (np.abs(t['m']) + np.abs(z).dot(np.abs(t['L']).T))
        err = np.abs(t['prop'] - exp)
        print('%s D=%d site %d: largest error / bound %.3e' % (model, D, k, (err / bound).max()))
        assert np.all(err <= bound)
    other = eng.site_evidence(seed=seed + 1, site0=site0, theta=theta, chains=4, with_terms=True)[1]
    assert np.all(other[0]['prop'] != terms[0]['prop']) and other[0]['L'].tobytes() == terms[0]['L'].tobytes()


# ------------------------------------------------------------------ 4. soft failures and refusals
def test_soft_failures_are_nan_records_of_that_site_only():
    model, D, rows, K = 'm4b_sg', 5, 17, 3
    X, y, k_lim, Oms, mus, d, P = _site_problem(model, D, rows, 43, K=K)
    eng, _, _ = _engine_with_cavity(model, X, y, k_lim, Oms, mus)
    theta = _draws(np.random.RandomState(9), K, 4, 32, P)
    clean = eng.site_evidence(seed=1, theta=theta, chains=4)[0]
    assert np.all(np.isfinite(clean))
    value = [ev.EV_LOGZ, ev.EV_LOGZ_IS, ev.EV_RE2, ev.EV_KHAT]

    def check(bad_theta, site):
        out = eng.site_evidence(seed=1, theta=bad_theta, chains=4)[0]
        assert np.all(np.isnan(out[site, value])) and out[site, ev.EV_ITERS] == 0 and out[site, ev.EV_N1] == 64
        others = [k for k in range(K) if k != site]
        assert out[others].tobytes() == clean[others].tobytes()

    bad = theta.copy()
    bad[1, 3 * 32 + 20, 4] = np.nan                      # one draw of E
    check(bad, 1)
    bad = theta.copy()
    bad[2, 5, 0] = np.inf                                # one draw of F: no factor
    check(bad, 2)
    bad = theta.copy()
    bad[0, :, P - 1] = bad[0, :, 2]                      # a duplicated coordinate: singular C
    check(bad, 0)
    assert np.array_equal(eng.site_evidence(seed=1, theta=theta, chains=4)[0], clean)        # and the context is fine


def _message(call):
    with pytest.raises(RuntimeError) as e:
        call()
    return str(e.value)


def test_refusals_come_before_any_launch():
    rng = np.random.RandomState(1)
    X, y, k_lim, Oms, mus, d, P = _site_problem('m4b_sg', 5, 4, 3, K=2)
    eng = HipEngine('m4b_sg', X, y, k_lim)
    assert 'no draws yet' in _message(lambda: eng.site_evidence())
    assert P == 18
    out = eng.site_evidence(theta=np.zeros((2, 4 * 18, P)), chains=4)[0]        # |F| = 36 = 2 P: admitted; C = 0: NaN
    assert np.all(np.isnan(out[:, ev.EV_LOGZ])) and np.all(out[:, ev.EV_N1] == 36)
    msg = _message(lambda: eng.site_evidence(theta=np.zeros((2, 4 * 17, P)), chains=4))
    assert 'the fit set holds 32 draws (the first 8 of each of 4 chains), the proposal of P = 18 coordinates needs at ' \
           'least 36' in msg
    assert 'S = 70 draws are no multiple of chains = 4' in _message(
        lambda: eng.site_evidence(theta=np.zeros((2, 70, P)), chains=4))
    _message(lambda: eng.site_evidence(theta=np.zeros((3, 80, P)), chains=4, k0=0, count=3))       # 3 of 2 sites
    # a P beyond the LDS limit, from sizes alone: before "no draws yet"
    D = 64
    big = HipEngine('m4b_sg', rng.randn(2, D), np.array([0, 1]), np.array([0, 1, 2]))
    assert big.P == 195 > ev.max_coords(D)
    assert 'P = 195 sampled coordinates, at most %d at D = 64' % ev.max_coords(D) in _message(lambda: big.site_evidence())
    ok = HipEngine('m4b_sg', rng.randn(2, 32), np.array([0, 1]), np.array([0, 1, 2]))
    assert ok.P == 99 and 'no draws yet' in _message(lambda: ok.site_evidence())          # m4b at D = 32 is admitted
    wide = HipEngine('m1b_sg', rng.randn(2, 129), np.array([0, 1]), np.array([0, 1, 2]))
    assert 'D = 129 columns, at most 128' in _message(lambda: wide.site_evidence())


# ------------------------------------------------------------------ 5. end to end
def test_master_log_evidence_on_the_device():
    M = teh.quad_master(_engine_factory=None)
    assert isinstance(M.engine, HipEngine)
    assert M.run(3, verbose=False, seed=4, calc_moments=False) == 0
    eng = M.engine
    before = (M.iter, M.dQi.copy(), M.dri.copy(), [eng.get_tilted(k) for k in range(2)],
              [eng.get_site(_engine.DQI, k) for k in range(2)])
    res = M.log_evidence(seed=5)
    exact, log_zk = teh.master_truth(M)
    print('log_evidence %.5f, quadrature %.5f; site_log_z %s, quadrature %s; re2 %s, khat %s, iters %s, %.3f ms'
          % (res['log_evidence'], exact, res['site_log_z'], log_zk, res['re2'], res['khat'], res['iters'], res['ms']))
    assert abs(res['log_evidence'] - exact) <= 6 * teh.SIGMA * np.sqrt(2)
    assert res['n_bad'] == 0 and np.all(res['iters'] <= 1000) and np.all(np.isfinite(res['khat']))
    assert M.iter == before[0] and np.array_equal(M.dQi, before[1]) and np.array_equal(M.dri, before[2])
    for k in range(2):
        for a, b in zip(before[3][k] + before[4][k], eng.get_tilted(k) + eng.get_site(_engine.DQI, k)):
            assert np.array_equal(np.asarray(a), np.asarray(b))
    assert eng.num_draws() == 1600
    # the draws the launch left, in the device's order, through the host statement
    out = eng.site_evidence(seed=5, site0=0)[0]
    # the caller's chains size the buffer of the terms: the library refuses any but the sampling call's
    assert 'chains = 2 given, the last sampling call left draws of 4 chains' in _message(
        lambda: eng.site_evidence(seed=5, site0=0, chains=2, with_terms=True))
    same, terms, _ = eng.site_evidence(seed=5, site0=0, chains=4, with_terms=True)
    assert same.tobytes() == out.tobytes() and terms[1]['l1'].shape == (800,) and terms[1]['prop'].shape == (800, 3)
    for k in range(2):
        sl = slice(int(M.k_lim[k]), int(M.k_lim[k + 1]))
        Om, mu = eng.get_cavity(k)
        rec = ev.site_evidence_host(0, 1, False, M.X[sl], M.y[sl], None, mu, Om,
                                    np.ascontiguousarray(eng.get_draws(k, all_params=True)), 4, 5, k)[0]
        np.testing.assert_allclose(out[k, COLS], rec[COLS], rtol=1e-8)
        assert out[k, ev.EV_ITERS] == rec[ev.EV_ITERS]
        assert res['site_log_z'][k] == ev.site_log_z(out[k, ev.EV_LOGZ], Om, 1, 0)
