"""A. The lean elementary functions of csrc/epx_device.h ON THEIR OWN, on the device, against long double.

epx_math_probe evaluates one of them per launch, elementwise, on the grids of lean_math_cases.py (test_lean_math_cases.py
checks without a device that the named edges are in the grids and that the np.longdouble reference agrees with 50-digit
mpmath to 2^-9 of every unit used here).  Error is counted in ulps of the double nearest to the true result (np.spacing:
2^-1074 where that is subnormal).  The budgets are the maxima of a double-precision emulation of the header over these
grids, plus one ulp; they are not taken from the device:

  rcp_d                       <= 0.51 ulp (the emulation rounds correctly for any seed error up to 5.9e-8)
  exp_d                       <= 1 ulp where the result is normal, <= 1 unit of 2^-1074 where it is subnormal; exactly
                              0 / inf / NaN at the listed points
  log1p_unit_d                <= 4 ulp while the function does not fold (1 + e not above sqrt 2), <= 3e-16 absolute above
  log_ge1_d                   <= 4 ulp; log_pos_d the same bits, and -inf at +-0
  log_sum_exp2[_lean], merge_weights' lse   <= 4 ulp of max(|result|, 1);  p_right <= 2 ulp
  logistic_terms / _split     g within 2.3e-16 absolute, ll within 4 ulp of max(|ll|, 1), w within 1 ulp of 1 + exp(-|f|)
  logistic_pair_lean          g within 2.3e-16 absolute, w the bits of logistic_split's, lin == y f - max(f, 0)

and, bit for bit: exp_d == exp_d_vc, log_ge1_d == log_ge1_d_vc, each slot of logistic_split2 == logistic_split in all
three outputs, logistic_pair_lean's w == logistic_split's w; the same call twice gives the same bytes.

Three places where the statement had to be made precise:
  * exp(-745.13) is 0.5016 x 2^-1074, which rounds to 2^-1074 and not to 0 (ln 2^-1075 = -745.13322): that point is held
    to the subnormal rule; "exactly 0" is asserted where the true result is below 2^-1075 (-745.14 and on).
  * p_right = e^b / (e^a + e^b) is formed from exp(fl(a - b)).  Where that difference rounds (|a| well below |b|), the
    rounding alone -- up to half an ulp of 800, 5.7e-14 -- is hundreds of ulps of a small probability: the 2 ulp are
    counted against the long-double value AT the double difference fl(b - a), the argument the function is given.  The
    error against the exact difference is printed beside it (the same on this grid: with |a| up to 1e4 nearly every
    difference is exact).
  * y f - max(f, 0) is not a number at f = +-inf (0 x inf, inf - inf): `lin` and `ll` are compared at finite f; at
    f = +-inf and NaN logistic_pair_lean's lin must be non-finite, which is how its caller learns of such a logit.

Measured on the device (MI355X, the maxima this test prints; the emulation gives the same figures to every digit
shown, with a reciprocal seed that is off by 2^-25):

  rcp_d                                   0.5000 ulp
  exp_d, normal results                   0.8638 ulp          (at x = -29.44)
  exp_d, subnormal results                0.8047 units of 2^-1074
  log1p_unit_d, not folded                2.986 ulp           (at e = 0.2689)
  log1p_unit_d, folded                    2.082e-16 absolute  (3.751 ulp, at e = 0.4604)
  log_ge1_d                               2.996 ulp           (at x = 1 + 8.6e-7)
  log_sum_exp2_lean, log_sum_exp2, merge_weights' lse     0.4995 ulp of max(|lse|, 1)
  merge_weights' p_right                  1.549 ulp
  logistic_terms, _split, _pair_lean g    1.653e-16 absolute  (at f = 14.97)
  logistic_terms ll                       1.255 ulp of max(|ll|, 1)
  logistic_split w                        0.8721 ulp

A finding of this test: logistic_terms formed ll as y f - (max(f, 0) + log1p(e^-|f|)).  For y = 1 and f > 0 the sum
rounds at half an ulp of f before f cancels -- 16 ulps of 1 at f = 33, where ll = -4.6e-15 (15.999 on this grid in the
emulation).  epx_device.h now subtracts y f - max(f, 0), which is exact, first: 1.255.

B. Every layout's log density and gradient where the logits saturate: test_logdensity_gradient_at_saturated_logits.
Measured: |lp - oracle| <= 1.8e-15 max(1, |lp|) and |g - oracle| <= 3.4e-15 max |g| over every case and layout (lp down
to -1.7e6, max |g| up to 8.1e5).
"""

import functools

import numpy as np
import pytest

import lean_math_cases as lm
from epstan_amd import _lib
from epstan_amd.engine import HipEngine
from oracle import nuts_oracle as no
from test_gpu_parity import _engine_with_cavity, _site_problem

pytestmark = pytest.mark.gpu

LD = np.longdouble
G_ABS = 2.3e-16                 # one ulp of 1: the residual y - sigmoid(f) carries an ABSOLUTE error


def _inputs(kind):
    if kind == 'rcp':
        return lm.rcp_grid(), None
    if kind in ('exp', 'exp_vc'):
        return lm.exp_grid(), None
    if kind == 'log1p_unit':
        return lm.log1p_grid(), None
    if kind in ('log_ge1', 'log_ge1_vc'):
        return lm.log_grid(), None
    if kind == 'log_pos':
        return lm.log_pos_grid(), None
    if kind in ('lse2_lean', 'lse2', 'merge'):
        a, b = lm.lse_grid()
        sa = np.array([c[0][0] for c in lm.LSE_SPECIAL]); sb = np.array([c[0][1] for c in lm.LSE_SPECIAL])
        return np.concatenate([a, sa]), np.concatenate([b, sb])
    return lm.logistic_grid()


@functools.lru_cache(maxsize=None)
def _probe(kind, call=0):
    """(n, 4) results of one launch; `call` distinguishes repeated launches of the same kind."""
    a, b = _inputs(kind)
    out = _lib.math_probe(kind, a, b)
    out.setflags(write=False)
    return out


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _assert_same_bits(x, y, what):
    bad = np.flatnonzero(_bits(x) != _bits(y))
    assert bad.size == 0, '%s: %d elements differ, the first at index %d: %r against %r' % (what, bad.size, bad[0], x.ravel()[bad[0]], y.ravel()[bad[0]])


def _report(name, err, unit, where=None):
    err = np.asarray(err, dtype=np.float64)
    i = int(np.argmax(err))
    print('measured %-34s max %.4g %s%s' % (name, err[i], unit, '' if where is None else ' at %r' % (where[i],)))
    return float(err[i])


# ---------------------------------------------------------------------------------------------------------- refusals
def test_probe_refuses_unknown_kinds_and_negative_counts():
    lib = _lib.load()
    a = np.ones(4); out = np.full((4, 4), 7.0)
    for kind in (-1, len(_lib.MATH_PROBE_KINDS), 1000):
        with pytest.raises(_lib.EpxError, match='unknown kind'):
            _lib.check(lib.epx_math_probe(0, kind, 4, _lib.dptr(a), _lib.dptr(a), _lib.dptr(out)))
    with pytest.raises(_lib.EpxError, match='n = -1'):
        _lib.check(lib.epx_math_probe(0, 0, -1, _lib.dptr(a), _lib.dptr(a), _lib.dptr(out)))
    assert np.all(out == 7.0)
    _lib.check(lib.epx_math_probe(0, 0, 0, None, None, None))                  # nothing to do is not an error
    # unused slots are 0, and a count that is no multiple of the block takes the tail
    x = np.linspace(1.0, 2.0, 257)
    r = _lib.math_probe('rcp', x)
    assert not r[:, 1:].any() and np.all(r[:, 0] > 0.49)
    assert len(_lib.MATH_PROBE_KINDS) == 16


# ---------------------------------------------------------------------------------------------------------- accuracy
def test_rcp_is_correctly_rounded():
    x = lm.rcp_grid()
    err = lm.err_ulps(_probe('rcp')[:, 0], lm.ref_rcp(x))
    assert _report('rcp_d', err, 'ulp', x) <= 0.51


def test_exp_in_ulps():
    x = lm.exp_grid()
    dev = _probe('exp')[:, 0]
    ref = lm.ref_exp(x)
    fin = np.isfinite(x)
    over = fin & (ref > LD(lm.DBL_MAX) * (1 + LD(2.0) ** -54))
    normal = fin & ~over & (ref >= lm.DBL_MIN)
    sub = fin & (ref < lm.DBL_MIN)
    assert normal.sum() > 65000 and sub.sum() >= 4900 and over.sum() == 4
    assert np.all(np.isfinite(dev[normal])) and np.all(dev[normal] > 0)
    e_n = _report('exp_d, normal results', lm.err_ulps(dev[normal], ref[normal]), 'ulp', x[normal])
    e_s = _report('exp_d, subnormal results', lm.err_in(dev[sub], ref[sub], lm.SUB_UNIT), 'units of 2^-1074', x[sub])
    assert e_n <= 1.0
    assert e_s <= 1.0
    assert np.all(dev[over] == np.inf)
    for v in lm.EXP_TO_ZERO:
        assert np.all(_bits(dev[_bits(x) == _bits(np.array([v]))[0]]) == 0), v      # +0, bit for bit
    for v in lm.EXP_TO_INF:
        assert np.all(dev[x == v] == np.inf), v
    assert np.all(dev[x == 0.0] == 1.0) and np.all(dev[np.abs(x) == 1e-300] == 1.0)
    assert np.isnan(x).sum() == 1 and np.all(np.isnan(dev[np.isnan(x)]))
    assert not np.isnan(dev[~np.isnan(x)]).any()


def test_log1p_unit_in_ulps():
    e = lm.log1p_grid()
    dev = _probe('log1p_unit')[:, 0]
    ref = lm.ref_log1p(e)
    big = (1.0 + e) > lm.SQRT2_CUT                       # the function's own branch: the same rounded sum
    assert big.sum() > 10000 and (~big).sum() > 10000
    e_lo = _report('log1p_unit_d, not folded', lm.err_ulps(dev[~big], ref[~big]), 'ulp', e[~big])
    e_hi = _report('log1p_unit_d, folded', lm.err_in(dev[big], ref[big], 1.0), 'absolute', e[big])
    _report('log1p_unit_d, folded', lm.err_ulps(dev[big], ref[big]), 'ulp', e[big])
    assert e_lo <= 4.0
    assert e_hi <= 3e-16
    assert dev[e == 0.0][0] == 0.0


def test_log_in_ulps_and_log_pos_is_log_ge1():
    x = lm.log_grid()
    dev = _probe('log_ge1')[:, 0]
    assert _report('log_ge1_d', lm.err_ulps(dev, lm.ref_log(x)), 'ulp', x) <= 4.0
    assert dev[x == 1.0][0] == 0.0
    pos = _probe('log_pos')[:, 0]
    n = x.shape[0]
    _assert_same_bits(pos[:n], dev, 'log_pos_d against log_ge1_d')
    assert lm.log_pos_grid().shape[0] == n + 2 and np.all(pos[n:] == -np.inf)


def _lse_check(kind):
    a, b = lm.lse_grid()
    n = a.shape[0]
    out = _probe(kind)
    ref = lm.ref_lse(a, b)
    err = _report({'lse2_lean': 'log_sum_exp2_lean', 'lse2': 'log_sum_exp2', 'merge': 'merge_weights lse'}[kind],
                  lm.err_in(out[:n, 0], ref, lm.ulp_of_max1(ref)), 'ulp of max(|lse|, 1)')
    assert err <= 4.0
    return out, n


@pytest.mark.parametrize('kind', ['lse2_lean', 'lse2'])
def test_log_sum_exp2_in_ulps(kind):
    out, n = _lse_check(kind)
    for i, ((a, b), want, _) in enumerate(lm.LSE_SPECIAL):
        assert out[n + i, 0] == want, (a, b)
    assert not out[:, 1:].any()


def test_merge_weights_in_ulps():
    out, n = _lse_check('merge')
    a, b = lm.lse_grid()
    d = b - a                                           # the double difference the function forms (fl(a - b) = -fl(b - a))
    ref = lm.ref_p_right(d)
    assert np.all(out[:n, 1] >= 0.0) and np.all(out[:n, 1] <= 1.0)
    err = _report('merge_weights p_right', lm.err_ulps(out[:n, 1], ref), 'ulp (at the double difference)', d)
    _report('merge_weights p_right', lm.err_ulps(out[:n, 1], lm.ref_p_right(LD(1) * b - LD(1) * a)), 'ulp (at the exact difference)', d)
    assert err <= 2.0
    for i, ((a1, b1), _, (lse, p)) in enumerate(lm.LSE_SPECIAL):
        np.testing.assert_array_equal(out[n + i, :2], [lse, p], err_msg=repr((a1, b1)))     # (NaN == NaN here)


def _logistic_check(name, ll, w, g, lin):
    """The outputs a logistic kind has, against the reference: ll and lin at finite f, w and g wherever f is a number."""
    f, y = lm.logistic_grid()
    ref = lm.ref_logistic(f, y)
    num, fin = ~np.isnan(f), np.isfinite(f)
    if g is not None:
        assert _report(name + ' g', lm.err_in(g[num], ref['g'][num], 1.0), 'absolute', f[num]) <= G_ABS
        assert np.all(np.isnan(g[~num])) or name.startswith('logistic_pair_lean')
    if w is not None:
        assert _report(name + ' w', lm.err_ulps(w[num], ref['w'][num]), 'ulp', f[num]) <= 1.0
        assert np.all(np.isnan(w[~num])) or name.startswith('logistic_pair_lean')
    if ll is not None:
        assert _report(name + ' ll', lm.err_in(ll[fin], ref['ll'][fin], lm.ulp_of_max1(ref['ll'][fin])), 'ulp of max(|ll|, 1)', f[fin]) <= 4.0
    if lin is not None:
        with np.errstate(all='ignore'):
            want = y * f - np.maximum(f, 0.0)           # exact in double for y = 0, 1 and finite f
        assert np.array_equal(lin[fin], want[fin]), name
        assert np.array_equal(LD(1) * want[fin], ref['lin'][fin])
    return f, y


def test_logistic_terms_and_split_against_long_double():
    t = _probe('terms')
    _logistic_check('logistic_terms', t[:, 0], None, t[:, 1], None)
    s = _probe('split')
    f, y = _logistic_check('logistic_split', None, s[:, 1], s[:, 2], s[:, 0])
    assert not t[:, 2:].any() and not s[:, 3].any()
    nan = np.isnan(f)
    assert nan.sum() == 4 and np.all(np.isnan(s[nan, 1])) and np.all(np.isnan(s[nan, 2])) and np.all(np.isnan(t[nan, 1]))
    # w == 1 exactly once exp(-|f|) is below half an ulp of 1, and w == 2 at f == 0
    assert np.all(s[np.abs(f) >= 37.0, 1] == 1.0) and np.all(s[f == 0.0, 1] == 2.0)
    assert np.all(s[f == 0.0, 2] == y[f == 0.0] - 0.5)


@pytest.mark.parametrize('slot', ['a', 'b'])
def test_logistic_pair_lean_against_long_double_and_split(slot):
    p = _probe('pair_lean_' + slot)
    s = _probe('split')
    f, y = _logistic_check('logistic_pair_lean ' + slot, None, None, p[:, 2], p[:, 0])
    fin = np.isfinite(f)
    _assert_same_bits(p[fin, 1], s[fin, 1], "logistic_pair_lean's w against logistic_split's")
    assert np.all(~np.isfinite(p[~fin, 0]))             # a logit that is not finite shows in lin
    assert np.all(np.isnan(p[np.isnan(f), 0]))
    assert not p[:, 3].any()


# ---------------------------------------------------------------------------------------------------------- one polynomial
def test_every_spelling_of_the_polynomials_gives_the_same_bits():
    _assert_same_bits(_probe('exp_vc')[:, 0], _probe('exp')[:, 0], 'exp_d_vc against exp_d')
    _assert_same_bits(_probe('log_ge1_vc')[:, 0], _probe('log_ge1')[:, 0], 'log_ge1_d_vc against log_ge1_d')
    s = _probe('split')
    for slot in ('a', 'b'):
        s2 = _probe('split2_' + slot)
        for j, name in enumerate(('lin', 'w', 'g')):
            _assert_same_bits(s2[:, j], s[:, j], 'logistic_split2 slot %s, %s, against logistic_split' % (slot, name))
    # ... and the exponential inside the logistic forms is exp_d's: the grid starts with f = -x and f = x for the exp
    # grid's x, and exp_d(-|f|) is exp_d(x) where x <= 0
    x = lm.exp_grid()
    nx = x.shape[0]
    neg = np.isfinite(x) & (x <= 0.0)
    for first in (0, nx):
        _assert_same_bits(s[first:first + nx, 1][neg], 1.0 + _probe('exp')[neg, 0], "logistic_split's w against 1 + exp_d(-|f|)")


def test_the_same_call_twice_gives_the_same_bytes():
    for kind in _lib.MATH_PROBE_KINDS:
        _assert_same_bits(_probe(kind, 1), _probe(kind), kind)


# ---------------------------------------------------------------------------------------------------------- B
RESIDENT_LAYOUTS = (1, 2, 4, 5, 6, 7)
SCALES = {'s1': 1.0, 's30': 30.0, 's400': 400.0, 's3000': 3000.0, 'theta0': 1.0}


def _shapes():
    """(model, D, n, layout requested, layout served)."""
    out = []
    for model in ('m1b_sg', 'm4b_sg', 'm2b_sg', 'm3b_sg', 'm5b_sg'):
        small = model in ('m1b_sg', 'm4b_sg')
        for D, n in [(4, 50), (32, 65), (16, 200)] if small else [(16, 200)]:
            for layout in RESIDENT_LAYOUTS:
                # layouts 5, 6, 7 exist for column paddings 16 and 32 only: at D = 4 they fall back, (9, 50) takes its place
                out.append((model, 9 if (D == 4 and layout >= 5) else D, n, layout, layout))
        for D, n in [(40, 150), (33, 70)] if small else [(40, 150)]:
            out.append((model, D, n, 0, 3))              # smoke()'s rule: the library itself must pick the streaming kernel
    return out


CASES = [(m, D, n, tag, req, served) for (m, D, n, req, served) in _shapes() for tag in SCALES]
CASES.sort(key=lambda c: (c[0], c[1], c[2], list(SCALES).index(c[3])))          # the layouts of a problem one after the other
_problem = {}


def _saturated_problem(model, D, n, tag):
    """Engine, oracle values and theta of one (model, shape, scale); kept for the layouts that follow."""
    key = (model, D, n, tag)
    if _problem.get('key') != key:
        _problem.clear()
        X, y, k_lim, Oms, mus, d, P = _site_problem(model, D, n, 100 + D)
        X = X * SCALES[tag]
        eng, Om_dev, mu_dev = _engine_with_cavity(model, X, y, k_lim, Oms, mus)
        theta = np.zeros(P) if tag == 'theta0' else np.random.RandomState(5).randn(P) * 0.5
        ref = [no.logdensity_grad(model, X[k_lim[k]:k_lim[k + 1]], y[k_lim[k]:k_lim[k + 1]], mu_dev[k], Om_dev[k], theta) for k in range(2)]
        _problem.update(key=key, eng=eng, theta=theta, ref=ref)
    return _problem


@pytest.mark.parametrize('model,D,n,tag,req,served', CASES, ids=['%s-%d-%d-%s-layout%d' % (c[0], c[1], c[2], c[3], c[5]) for c in CASES])
def test_logdensity_gradient_at_saturated_logits(model, D, n, tag, req, served):
    """test_logdensity_gradient_matches_oracle's set-up with the rows scaled by s = 1 (control), 30 (most rows have
    w == 1 exactly), 400 (subnormal exp and the clamp at -800), 3000 (every row clamped, |f| ~ 1e4), and theta = 0 at
    s = 1 (every f == 0, w == 2 in every factor: the largest product of w's a lane can form), on every layout -- the
    first direct gradient test of layout 4.  Shapes: (4, 50), (32, 65), (16, 200) on the resident layouts -- layouts 5,
    6, 7 are built for column paddings 16 and 32 only and fall back at D = 4, so (9, 50) stands in for (4, 50) there --
    and (40, 150), (33, 70) streamed (layout 0 must report 3).  Bounds: the ones the existing tests of the same hook
    use, every atol scaled by max |g|.  The oracle is finite at every case; two calls give the same bits."""
    p = _saturated_problem(model, D, n, tag)
    eng, theta = p['eng'], p['theta']
    lp_tol, g_tol = {1: (1e-11, 1e-10), 2: (1e-11, 1e-10), 5: (1e-11, 1e-10), 6: (1e-11, 1e-10), 7: (1e-9, 1e-9),
                     3: (1e-10, 1e-9), 4: (1e-10, 1e-9)}[served]
    for k in range(2):
        lp_o, g_o = p['ref'][k]
        assert np.isfinite(lp_o) and np.all(np.isfinite(g_o))
        lp, g = eng.logdensity_grad(k, theta, layout=req)
        assert eng.last_layout() == served, (req, eng.last_layout())
        lp2, g2 = eng.logdensity_grad(k, theta, layout=req)
        assert lp2 == lp and np.array_equal(g2, g)
        gmax = max(1.0, np.abs(g_o).max())
        print('%s D=%d n=%d %s layout %d site %d: lp %.6g diff %.2e (rel), max|g| %.3g diff %.2e (of max|g|)'
              % (model, D, n, tag, served, k, lp_o, abs(lp - lp_o) / max(1.0, abs(lp_o)), gmax, np.abs(g - g_o).max() / gmax))
        assert abs(lp - lp_o) <= lp_tol * max(1.0, abs(lp_o))
        np.testing.assert_allclose(g, g_o, rtol=g_tol, atol=g_tol * gmax)
