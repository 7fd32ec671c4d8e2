"""k_reweight / epx_reweight_batch / HipEngine.reweight_batch / Worker.tilted_reuse / Master.run(reuse=...) on the device:
the tilted moments under a moved cavity from the draws sampled against the old one, by Pareto-smoothed importance sampling
(include/epx.h: epx_reweight_batch; reweight.py restates it in NumPy).

Bounds.  Mean, scatter, KHAT and WESS against reweight_host on the same inputs: the derived bound of
test_gpu_loo._psis_check -- 100 x the largest |float64 - longdouble| of the host statement for that output over the case,
with a floor of 1e-12 x the output's largest magnitude; the smoothed / not-smoothed pattern must agree exactly.  dQi, dri:
the host's precision estimate applied to the DEVICE's own mean, scatter and n, rtol = atol = 1e-8 (test_gpu_parity's bound
for the same code).  Measured on an MI355X, largest error / bound over test 1: mean 1.0e-3, scatter
2.9e-3, WESS 3.2e-3, KHAT 5.8e-2; dQi, dri: largest error 5.8e-15."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from epstan_amd import _lib, models, reweight                   # noqa: E402
from epstan_amd.engine import HipEngine, DQI                    # noqa: E402
from epstan_amd.method import Master, Worker                    # noqa: E402
from test_gpu_parity import _site_problem                       # noqa: E402

KHAT, WESS = reweight.RW_KHAT, reweight.RW_WESS
N_ROWS = 7
SHAPES = [('m1b_sg', 3, 4, 20), ('m1b_sg', 3, 4, 25), ('m1b_sg', 3, 4, 64), ('m4b_sg', 8, 18, 64), ('m4b_sg', 8, 18, 203),
          ('m4b_sg', 16, 34, 203), ('m4b_sg', 50, 102, 400)]


class Case(object):
    """K = 2 sites of `model` whose device cavities are the NEW ones, a global (Q, r), and draws with their OLD cavities."""

    def __init__(self, model, D, d, S, scale):
        X, y, k_lim, _, _, dd, P = _site_problem(model, D, N_ROWS, 100 + D, K=2)
        assert dd == d
        rng = np.random.RandomState(1000 * d + S)
        self.d, self.S, self.P, self.K = d, S, P, 2
        Oms, mus, On, mn = [], [], [], []
        self.theta = 0.2 * np.random.RandomState(S).randn(2, S, P)
        for k in range(2):
            A = rng.randn(d, d + 3)
            Oms.append(A.dot(A.T) / (d + 3) + 0.5 * np.eye(d))
            mus.append(0.5 * rng.randn(d))
            B = rng.randn(d, d)
            On.append(Oms[k] * (1 + scale) + scale * 0.1 * (B + B.T) / np.sqrt(d))
            mn.append(mus[k] + scale * rng.randn(d))
            L = np.linalg.cholesky(np.linalg.inv(Oms[k] + 2 * np.eye(d)))
            self.theta[k, :, :d] = 0.3 * mus[k] + rng.randn(S, d).dot(L.T)
        self.Oo, self.mo = np.array(Oms), np.array(mus)
        self.eng = HipEngine(model, X, y, k_lim)
        self.set_cavities(On, mn)
        G = rng.randn(d, d + 3)
        self.Q = np.asfortranarray(G.dot(G.T) / (d + 3) + np.eye(d))
        self.r = self.Q.dot(0.2 * rng.randn(d))
        self.eng.set_global(self.Q, self.r)

    def set_cavities(self, Om, mu):
        """Device cavities (Om[k], mu[k]) up to rounding; self.On, self.mn: what the device holds."""
        d = self.d
        for k in range(2):
            assert self.eng.cavity_site(k, Om[k] + np.eye(d), Om[k].dot(mu[k]), np.eye(d), np.zeros(d))
        self.On = np.stack([self.eng.get_cavity(k)[0] for k in range(2)])
        self.mn = np.stack([self.eng.get_cavity(k)[1] for k in range(2)])
        if hasattr(self, 'Q'):
            self.eng.set_global(self.Q, self.r)

    def call(self, prec_estim, theta=None, **kw):
        """Everything a call leaves behind, as one dict of arrays."""
        theta = self.theta if theta is None else theta
        k0, count = kw.get('k0', 0), kw.get('count', 2)
        sl = slice(k0, k0 + count)
        flags, rec, ms = self.eng.reweight_batch(prec_estim, theta=theta[sl], Om_old=self.Oo[sl], mu_old=self.mo[sl], **kw)
        return collect(self.eng, flags, rec, k0, count)

    def host(self, k, prec_estim, dtype=np.float64, theta=None):
        theta = self.theta if theta is None else theta
        return reweight.reweight_host(theta[k, :, :self.d].astype(dtype), self.Oo[k], self.mo[k], self.On[k], self.mn[k],
                                      self.Q, self.r, prec_estim)

    def close(self):
        self.eng.close()


def collect(eng, flags, rec, k0, count):
    out = dict(flags=flags.copy(), rec=rec.copy(), mean=[], scatter=[], dQi=[], dri=[], nsamp=[])
    for k in range(k0, k0 + count):
        Mat, vec, n = eng.get_tilted(k)
        dQ, dr = eng.get_site(DQI, k)
        out['mean'].append(vec); out['scatter'].append(Mat); out['dQi'].append(dQ); out['dri'].append(dr)
        out['nsamp'].append(n)
    return dict((key, np.array(v)) for key, v in out.items())


def same_bytes(a, b, sites_a=slice(None), sites_b=slice(None)):
    return all(np.ascontiguousarray(a[key][sites_a]).tobytes() == np.ascontiguousarray(b[key][sites_b]).tobytes()
               for key in ('flags', 'rec', 'mean', 'scatter', 'dQi', 'dri'))


def derived_check(what, got, host, wide):
    """got (device), host (float64), wide (longdouble): dicts of mean, scatter, khat, wess stacked over the sites of the
    case.  Returns {output: largest error / bound}."""
    raw = np.isinf(np.asarray(host['khat'], dtype=np.float64))
    assert np.array_equal(raw, np.isinf(np.asarray(wide['khat']).astype(np.float64))), what
    assert np.array_equal(raw, np.isposinf(got['khat'])), what + ': not-smoothed sites are exactly +inf in KHAT'
    ratios = {}
    for name in ('mean', 'scatter', 'khat', 'wess'):
        g, h, w = (np.asarray(v[name]) for v in (got, host, wide))
        assert not np.any(np.isnan(g)), (what, name)
        use = ~raw if name == 'khat' else np.ones(len(raw), dtype=bool)
        if not use.any():
            continue
        g, h, w = g[use].astype(np.float64), h[use].astype(np.float64), w[use]
        ref = float(np.abs((h - w).astype(np.float64)).max())
        bound = max(100.0 * ref, 1e-12 * float(np.abs(h).max()))
        err = float(np.abs(g - h).max())
        print('%s %s: largest error %.3e, float64 - longdouble %.3e, error / bound %.3e' % (what, name, err, ref, err / bound))
        ratios[name] = err / bound
        assert err <= bound, '%s %s: error %.3e, bound %.3e' % (what, name, err, bound)
    return ratios


def check_against_host(case, got, prec_estim, what, theta=None):
    host = [case.host(k, prec_estim, theta=theta) for k in range(2)]
    with np.errstate(all='ignore'):
        wide = [case.host(k, prec_estim, np.longdouble, theta=theta) for k in range(2)]
    stack = lambda rows: dict((n, np.stack([np.asarray(r[n]) for r in rows])) for n in ('mean', 'scatter', 'khat', 'wess'))
    dev = dict(mean=got['mean'], scatter=got['scatter'], khat=got['rec'][:, KHAT], wess=got['rec'][:, WESS])
    ratios = derived_check(what, dev, stack(host), stack(wide))
    assert got['nsamp'].tolist() == [case.S, case.S]
    for k in range(2):
        # the precision estimate: the host's on the device's own mean, scatter and n
        dQi, dri, ok = reweight.precision_host(got['mean'][k], got['scatter'][k], got['rec'][k, WESS], case.Q, case.r, prec_estim)
        assert bool(got['flags'][k]) == ok, (what, k)
        np.testing.assert_allclose(got['dQi'][k], dQi, rtol=1e-8, atol=1e-8, err_msg=what)
        np.testing.assert_allclose(got['dri'][k], dri, rtol=1e-8, atol=1e-8, err_msg=what)
        if ok:
            print('%s site %d: dQi error %.3e of %.3e, dri error %.3e' % (
                what, k, np.abs(got['dQi'][k] - dQi).max(), np.abs(dQi).max(), np.abs(got['dri'][k] - dri).max()))
    return ratios, host


# ------------------------------------------------------------------ 1. parity with the host statement
@pytest.mark.parametrize('scale', [0.02, 0.1])
@pytest.mark.parametrize('model,D,d,S', SHAPES)
def test_reweight_matches_the_host_on_injected_draws(model, D, d, S, scale):
    case = Case(model, D, d, S, scale)
    try:
        full = None
        for prec_estim in ('sample', 'olse'):
            got = case.call(prec_estim)
            what = '%s d=%d S=%d scale=%g %s' % (model, d, S, scale, prec_estim)
            _, host = check_against_host(case, got, prec_estim, what)
            assert all(np.isposinf(h['khat']) for h in host) == (S == 20)        # M = 4: nothing is smoothed
            if S > 20:
                assert all(np.isfinite(h['khat']) for h in host)
                assert got['flags'].all()
            assert same_bytes(got, case.call(prec_estim))                          # twice: the same bytes
            full = got
        assert same_bytes(case.call('olse', k0=1, count=1), full, sites_b=slice(1, 2))
    finally:
        case.close()


# ------------------------------------------------------------------ 2. identical cavities
@pytest.mark.parametrize('prec_estim', ['sample', 'olse'])
@pytest.mark.parametrize('model,D,d,S', [SHAPES[0], SHAPES[4], SHAPES[6]])
def test_identical_cavities_give_the_moment_stage(model, D, d, S, prec_estim):
    case = Case(model, D, d, S, 0.1)
    try:
        eng = case.eng
        flags, rec, _ = eng.reweight_batch(prec_estim, theta=case.theta, Om_old=case.On, mu_old=case.mn)
        got = collect(eng, flags, rec, 0, 2)
        samples = np.asfortranarray(np.transpose(case.theta[:, :, :d], (1, 2, 0)))
        ref_flags = eng.moments_batch(samples, prec_estim)
        ref = collect(eng, ref_flags, np.zeros((2, 2)), 0, 2)
        assert got['flags'].tolist() == ref['flags'].tolist() == [True, True]
        assert np.all(np.isposinf(got['rec'][:, KHAT]))
        np.testing.assert_allclose(got['rec'][:, WESS], S, rtol=1e-12)
        for key in ('mean', 'scatter', 'dQi', 'dri'):
            np.testing.assert_allclose(got[key], ref[key], rtol=1e-12, atol=1e-12 * np.abs(ref[key]).max(), err_msg=key)
    finally:
        case.close()


# ------------------------------------------------------------------ 3. the draws and cavities of the last sampling call
def _sampled_engine(reuse):
    X, y, k_lim, Oms, mus, d, P = _site_problem('m1b_sg', 3, N_ROWS, 103, K=2)
    eng = HipEngine('m1b_sg', X, y, k_lim)
    for k in range(2):
        assert eng.cavity_site(k, Oms[k] + np.eye(d), Oms[k].dot(mus[k]), np.eye(d), np.zeros(d))
    if reuse:
        eng.set_draw_reuse(True)
    eng.sample_batch(np.array([5, 6]), HipEngine.sampler_opts(chains=4, iter=40))
    return eng, Oms, mus, d


def test_snapshot_path_is_the_injected_path():
    eng, Oms, mus, d = _sampled_engine(True)
    try:
        S = eng.num_draws()
        assert S == 80
        old = [eng.get_cavity(k) for k in range(2)]
        theta = np.stack([np.ascontiguousarray(eng.get_draws(k, all_params=True)) for k in range(2)])
        Q = np.asfortranarray(Oms[0] + 2 * np.eye(d))
        r = Q.dot(mus[0])
        eng.set_global(Q, r)
        # the cavity unmoved: uniform weights
        flags, rec, ms = eng.reweight_batch('sample')
        assert flags.all() and np.all(np.isposinf(rec[:, KHAT])) and ms > 0
        np.testing.assert_allclose(rec[:, WESS], S, rtol=1e-12)
        # moved
        for k in range(2):
            Om = Oms[k] * 1.05 + 0.01
            assert eng.cavity_site(k, Om + np.eye(d), Om.dot(mus[k] + 0.03), np.eye(d), np.zeros(d))
        eng.set_global(Q, r)
        flags, rec, _ = eng.reweight_batch('sample')
        snap = collect(eng, flags, rec, 0, 2)
        assert np.all(rec[:, WESS] < S)
        for k in range(2):
            new = eng.get_cavity(k)
            h = reweight.reweight_host(theta[k, :, :d], old[k][0], old[k][1], new[0], new[1], Q, r, 'sample')
            assert np.isinf(h['khat']) == np.isinf(rec[k, KHAT])
            np.testing.assert_allclose(rec[k, WESS], h['wess'], rtol=1e-9)
        flags, rec, _ = eng.reweight_batch('sample', theta=theta, Om_old=np.stack([o[0] for o in old]),
                                           mu_old=np.stack([o[1] for o in old]))
        assert same_bytes(snap, collect(eng, flags, rec, 0, 2))
        flags, rec, _ = eng.reweight_batch('sample', k0=1, count=1)
        assert same_bytes(snap, collect(eng, flags, rec, 1, 1), sites_a=slice(1, 2))
        # a sampling call of one site leaves the snapshot of that site only
        eng.sample_batch(np.array([7]), HipEngine.sampler_opts(chains=4, iter=40), k0=1, count=1)
        eng.reweight_batch('sample', k0=1, count=1)
        with pytest.raises(_lib.EpxError):
            eng.reweight_batch('sample')
    finally:
        eng.close()


def test_without_draw_reuse_the_call_names_the_switch():
    eng, _, _, _ = _sampled_engine(False)
    try:
        with pytest.raises(_lib.EpxError, match='epx_set_draw_reuse'):
            eng.reweight_batch('sample')
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. soft failure and bad data
@pytest.mark.parametrize('model,D,d,S', [SHAPES[3], SHAPES[5]])
def test_small_effective_sample_fails_softly_under_sample(model, D, d, S):
    case = Case(model, D, d, S, 0.3)
    try:
        got = case.call('sample')
        _, host = check_against_host(case, got, 'sample', 'd=%d S=%d scale=0.3 sample' % (d, S))
        assert all(float(h['wess']) - d - 2 < 0 for h in host)
        assert got['flags'].tolist() == [False, False]
        assert not got['dQi'].any() and not got['dri'].any()
        assert np.all(np.isfinite(got['mean'])) and np.all(np.isfinite(got['rec']))
    finally:
        case.close()


def test_a_nan_draw_voids_its_site_only():
    model, D, d, S = SHAPES[4]
    case = Case(model, D, d, S, 0.1)
    try:
        clean = case.call('olse')
        theta = case.theta.copy()
        theta[0, 5, 2] = np.nan
        got = case.call('olse', theta=theta)
        assert np.all(np.isnan(got['rec'][0])) and not got['flags'][0]
        assert not got['dQi'][0].any() and not got['dri'][0].any()
        assert same_bytes(got, clean, sites_a=slice(1, 2), sites_b=slice(1, 2))
        host = case.host(0, 'olse', theta=theta)
        assert np.isnan(host['khat']) and not host['ok']
    finally:
        case.close()


# ------------------------------------------------------------------ 5. refusals in front of the first copy
def test_refusals_leave_the_context_untouched():
    model, D, d, S = SHAPES[1]
    case, fresh = Case(model, D, d, S, 0.1), Case(model, D, d, S, 0.1)
    try:
        eng = case.eng
        with pytest.raises(_lib.EpxError, match='site range'):
            eng.reweight_batch('sample', k0=1, count=2, theta=case.theta, Om_old=case.Oo, mu_old=case.mo)
        with pytest.raises(_lib.EpxError, match='fewer draws'):
            eng.reweight_batch('sample', theta=case.theta[:, :d - 1], Om_old=case.Oo, mu_old=case.mo)
        with pytest.raises(_lib.EpxError, match='Om_old'):
            eng.reweight_batch('sample', theta=case.theta)
        with pytest.raises(_lib.EpxError, match='Om_old'):
            eng.reweight_batch('sample', theta=case.theta, Om_old=case.Oo)
        with pytest.raises(_lib.EpxError, match='prec_estim'):
            eng.reweight_batch(7, theta=case.theta, Om_old=case.Oo, mu_old=case.mo)
        with pytest.raises(_lib.EpxError, match='no draws yet'):
            eng.reweight_batch('sample')
        assert same_bytes(case.call('sample'), fresh.call('sample'))
    finally:
        case.close()
        fresh.close()


# ------------------------------------------------------------------ 6. Master.run(reuse=...) and Worker.tilted_reuse
def _master():
    mod = models.m1b(4, 3, 40)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    return Master('m1b_sg', data.X, data.y, site_sizes=data.Nj, prior={'Q': Q0, 'r': r0}, chains=4, iter=60,
                  df0=0.5)


def test_run_with_a_policy_that_never_reuses_is_the_plain_run():
    plain, never = _master(), _master()
    assert plain.run(3, verbose=False, calc_moments=False, seed=3) == 0
    assert never.run(3, verbose=False, calc_moments=False, seed=3, reuse=dict(k_max=-np.inf)) == 0
    for name in ('Q', 'r', 'Qi', 'ri'):
        assert getattr(plain, name).tobytes() == getattr(never, name).tobytes(), name
    assert len(never.reuse_log) == 3 and not any(e['reused'] for e in never.reuse_log)
    assert never.reuse_log[1]['n_ok'] == 0 and never.reuse_log[1]['ms'] > 0
    assert len(never.sampling_ms) == 3 and plain.reuse_log == []


def test_run_with_a_policy_that_always_reuses_samples_once():
    always, first = _master(), _master()
    policy = dict(k_max=np.inf, min_ess=0)
    info, _, (stimes, msteps, mrhats, _) = always.run(3, verbose=False, seed=3, reuse=policy, return_analytics=True)
    assert info == 0 and len(always.sampling_ms) == 1
    assert [e['reused'] for e in always.reuse_log] == [False, True, True]
    assert all(e['n_ok'] == 4 and 0 < e['wess_min_frac'] <= 1 for e in always.reuse_log[1:])
    assert msteps[1] == msteps[0] and mrhats[2] == mrhats[0]
    np.testing.assert_allclose(stimes[1], always.reuse_log[1]['ms'] * 1e-3, rtol=1e-12)

    # iteration 2's update against the host statement on iteration 1's draws and the two cavities
    two = _master()
    assert two.run(2, verbose=False, calc_moments=False, seed=3, reuse=policy) == 0 and len(two.sampling_ms) == 1
    eng = first.engine
    old = [eng.get_cavity(k) for k in range(4)]
    assert first.run(1, verbose=False, calc_moments=False, seed=3) == 0
    Q, r = eng.get_global()
    d = eng.d
    host, wide, dev = [], [], dict(mean=[], scatter=[])
    for k in range(4):
        phi = np.ascontiguousarray(eng.get_draws(k))
        new = eng.get_cavity(k)
        host.append(reweight.reweight_host(phi, old[k][0], old[k][1], new[0], new[1], Q, r, 'sample'))
        with np.errstate(all='ignore'):
            wide.append(reweight.reweight_host(phi.astype(np.longdouble), old[k][0], old[k][1], new[0], new[1], Q, r, 'sample'))
        Mat, vec, n = two.engine.get_tilted(k)
        assert n == phi.shape[0] == 120
        dev['mean'].append(vec); dev['scatter'].append(Mat)
    stack = lambda rows, names: dict((n, np.stack([np.asarray(v[n]) for v in rows])) for n in names)
    names = ('mean', 'scatter', 'khat', 'wess')
    h, w = stack(host, names), stack(wide, names)
    g = dict(mean=np.stack(dev['mean']), scatter=np.stack(dev['scatter']), khat=h['khat'].astype(np.float64),
             wess=h['wess'].astype(np.float64))          # (the run logs the extremes of khat and wess only)
    derived_check('Master.run iteration 2', g, h, w)
    log = two.reuse_log[1]
    finite = h['khat'][np.isfinite(h['khat'])]
    if finite.size:
        np.testing.assert_allclose(log['khat_max'], finite.max(), rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(log['wess_min_frac'], h['wess'].min() / 120, rtol=1e-9)
    for k in range(4):
        dQi, dri, ok = reweight.precision_host(g['mean'][k], g['scatter'][k], float(h['wess'][k]), Q, r, 'sample')
        assert ok
        np.testing.assert_allclose(two.dQi[:, :, k], dQi, rtol=1e-8, atol=1e-8)
        np.testing.assert_allclose(two.dri[:, k], dri, rtol=1e-8, atol=1e-8)


def test_worker_tilted_reuse_agrees_with_the_batch_call():
    X, y, k_lim, Oms, mus, d, P = _site_problem('m1b_sg', 3, N_ROWS, 103, K=1)
    moved = Oms[0] * 1.05 + 0.01
    for reuse in (True, False):
        w = Worker(0, 'm1b_sg', d, X, y, chains=4, iter=40)
        eng = w._eng
        try:
            dQi, dri = np.zeros((d, d), order='F'), np.zeros(d)
            with pytest.raises(RuntimeError):
                w.tilted_reuse(dQi, dri)                # no cavity yet
            assert w.cavity(Oms[0] + np.eye(d), Oms[0].dot(mus[0]), np.eye(d), np.zeros(d))
            with pytest.raises(_lib.EpxError, match='no draws yet'):
                w.tilted_reuse(dQi, dri)
            if reuse:
                eng.set_draw_reuse(True)
            assert w.tilted(dQi, dri, seed=5)
            Q, r = moved + np.eye(d), moved.dot(mus[0] + 0.03)
            assert w.cavity(Q, r, np.eye(d), np.zeros(d)) and w.phase == 1
            if not reuse:
                with pytest.raises(_lib.EpxError, match='epx_set_draw_reuse'):
                    w.tilted_reuse(dQi, dri)
                continue
            ok, khat, wess = w.tilted_reuse(dQi, dri)
            assert ok and w.phase == 2 and w.nsamp == 80 and w.iteration == 2
            assert 0 < wess < 80
            flags, rec, _ = eng.reweight_batch('sample', k0=0, count=1)
            assert (khat, wess) == (rec[0, KHAT], rec[0, WESS]) and flags[0]
            dQ, dr = eng.get_site(DQI, 0)
            assert np.array_equal(dQi, dQ) and np.array_equal(dri, dr) and dQ.any()
            Mat, vec, _ = eng.get_tilted(0)
            assert np.array_equal(w.Mat, Mat) and np.array_equal(w.vec, vec)
        finally:
            eng.close()
