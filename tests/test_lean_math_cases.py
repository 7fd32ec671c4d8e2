"""The grids and the long-double reference of lean_math_cases.py, checked without a device: every named edge is in the
array the device test runs, the grids have the stated extent, and the reference agrees with 50-digit mpmath to 2^-9 of
the unit each device assertion counts in -- so a device error of "0.86 ulp" is 0.86 +- 0.002, not an artefact of the
yardstick.  No mpmath values are stored: they are recomputed here (a few seconds)."""

import numpy as np
import pytest

import lean_math_cases as lm

LD = np.longdouble
REF_TOL = 2.0 ** -9


def test_long_double_has_a_64_bit_mantissa():
    """The reference is only better than the device's doubles where long double is the x87 format."""
    assert np.finfo(LD).nmant >= 63 and np.finfo(LD).maxexp >= 16384


# ---------------------------------------------------------------------------------------------------------- the grids
def test_exp_grid_holds_its_edges():
    x = lm.exp_grid()
    for v in lm.EXP_EDGES:
        assert lm.holds(x, v), v
    for v in lm._neighbours(lm.exp_boundaries()):
        assert lm.holds(x, v)
    assert lm.EXP_K[0] == -1000 and lm.EXP_K[-1] == 1000 and lm.EXP_K.shape[0] == 2001
    # the boundaries are boundaries: the nearest integer to x / ln 2 changes from k to k + 1 across (k + 1/2) ln 2
    b = lm.exp_boundaries()
    q = (LD(1) * b) / np.log(LD(2))
    assert np.all(np.abs(q - (lm.EXP_K + LD(0.5))) < 1e-12)
    fin = x[np.isfinite(x)]
    ref = lm.ref_exp(fin)
    assert np.sum((ref < lm.DBL_MIN) & (ref >= lm.SUB_UNIT / 2)) >= 4900          # subnormal results
    assert np.sum((fin >= -0.35) & (fin <= 0.35)) >= 20000 and np.sum(np.abs(fin) <= 40.0) >= 40000
    # what the listed points do: true results below half of 2^-1074, the one just above it, and overflow
    half = LD(lm.SUB_UNIT) / 2
    assert np.all(lm.ref_exp(np.array(lm.EXP_TO_ZERO)) < half)
    last = lm.ref_exp(np.array(lm.EXP_LAST_SUBNORMAL)) / LD(lm.SUB_UNIT)
    assert np.all((last > 0.5) & (last < 0.51))                                  # rounds to 2^-1074, not to 0
    assert np.all(lm.ref_exp(np.array(lm.EXP_TO_INF)) > LD(lm.DBL_MAX) * (1 + LD(2.0) ** -54))
    assert np.all(lm.ref_exp(fin[(fin >= -708.3) & (fin <= 709.7)]) <= lm.DBL_MAX)


def test_log1p_grid_holds_its_edges():
    e = lm.log1p_grid()
    for v in lm.LOG1P_EDGES:
        assert lm.holds(e, v), v
    assert e.min() == 0.0 and e.max() == 1.0
    assert abs(LD(lm.FOLD) - (np.sqrt(LD(2)) - 1)) <= 2.0 ** -55                 # the double nearest to sqrt2 - 1
    # ... and the two doubles between which the function's own branch (1 + e, ROUNDED, above the cut) changes sides
    lo, hi = lm.log1p_branch_pair()
    assert hi == np.nextafter(lo, 2.0) and not (1.0 + lo) > lm.SQRT2_CUT and (1.0 + hi) > lm.SQRT2_CUT
    assert abs(lo - lm.FOLD) < 1e-15
    assert np.sum(np.abs(e - lm.FOLD) < 0.011) >= 2000 and np.sum(e < 1e-100) >= 1000


def test_log_grid_holds_its_edges():
    x = lm.log_grid()
    for v in lm.LOG_EDGES:
        assert lm.holds(x, v), v
    assert x.min() == lm.DBL_MIN and x.max() == lm.DBL_MAX                       # no subnormal argument
    assert np.sum(np.abs(x - 1.0) <= 1e-6) >= 3000 and np.sum((x >= 0.5) & (x <= 2.0)) >= 30000
    # the k = -1 cancellation: arguments whose mantissa is doubled, right below 1/sqrt2
    assert np.sum((x >= 0.5) & (x < lm.INV_SQRT2_CUT)) >= 1000
    xp = lm.log_pos_grid()
    for v in lm.LOG_EDGES + lm.LOG_POS_EDGES:
        assert lm.holds(xp, v), v


def test_rcp_and_lse_grids_have_their_extent():
    x = lm.rcp_grid()
    assert np.sum((x >= 1.0) & (x <= 2.0)) >= 30000 and x.min() < 2.0 ** -990 and x.max() > 2.0 ** 990
    assert np.all(np.isfinite(x)) and x.min() >= 2.0 ** -1000
    a, b = lm.lse_grid()
    assert a.shape == (10000,) and np.abs(a).max() <= 1e4 and np.abs(a - b).max() <= 800.0 + 1e-9
    assert np.abs(a - b).max() > 790.0 and np.abs(a - b).min() < 0.5


def test_logistic_grid_mirrors_the_exp_grid():
    f, y = lm.logistic_grid()
    assert set(np.unique(y)) == {0.0, 1.0}
    for yy in (0.0, 1.0):
        fy = f[y == yy]
        for v in lm.LOGISTIC_EXTRA:
            assert lm.holds(fy, v) and lm.holds(fy, -v), v
        for v in (0.0, -0.0, np.inf, -np.inf, np.nan, 745.13, -745.13, 800.0, -801.0):
            assert lm.holds(fy, v), v
        fin = np.sort(fy[np.isfinite(fy)])
        np.testing.assert_array_equal(fin, -fin[::-1])                          # every logit with both signs
    x = lm.exp_grid()
    assert f.shape[0] == 4 * (x.shape[0] + len(lm.LOGISTIC_EXTRA))
    # 36.0436 is just inside 52 ln 2: exp(-|f|) is the last bit of w there, and w == 1 exactly from 53 ln 2 = 36.74 on
    assert float(lm.ref_logistic(36.0436, 0.0)['w'].astype(np.float64)) == 1.0 + 2.0 ** -52
    assert float(lm.ref_logistic(-37.0, 1.0)['w'].astype(np.float64)) == 1.0


# ---------------------------------------------------------------------------------------------------------- the reference
def _worst(mpmath, ref, exact, unit):
    """max |ref - exact| / unit over the points.  Each exact value, scaled by the power of two that brings the reference
    into [1/2, 1), is split into a double and a remainder (a double too), so that the difference is formed in long double
    without loss whatever the size of the result (exp reaches 1e-4951 here, far below the doubles)."""
    ref = np.atleast_1d(ref)
    with np.errstate(all='ignore'):
        m, ex = np.frexp(ref)
    hi, lo = np.empty(ref.shape[0]), np.empty(ref.shape[0])
    for i, (t, k) in enumerate(zip(exact, ex)):
        s = mpmath.ldexp(t, -int(k))
        hi[i] = float(s)
        lo[i] = float(s - hi[i])
    with np.errstate(all='ignore'):
        err = np.ldexp(np.abs((m - LD(1) * hi) - LD(1) * lo), ex) / (LD(1) * np.atleast_1d(unit))
    assert np.all(np.isfinite(err))
    return float(err.max())


@pytest.fixture
def mpmath():
    mp = pytest.importorskip('mpmath')
    with mp.workdps(50):
        yield mp


def _finite(x):
    return x[np.isfinite(x)]


def test_reference_exp_agrees_with_mpmath(mpmath):
    x = _finite(lm.exp_grid())
    x = x[x < 709.78]                                                           # (beyond: the double result is inf)
    ref = lm.ref_exp(x)
    assert _worst(mpmath, ref, [mpmath.exp(mpmath.mpf(float(v))) for v in x], lm.ulp_of(ref)) <= REF_TOL


def test_reference_log1p_log_rcp_agree_with_mpmath(mpmath):
    e = lm.log1p_grid()
    ref = lm.ref_log1p(e)
    assert _worst(mpmath, ref, [mpmath.log1p(mpmath.mpf(float(v))) for v in e], lm.ulp_of(ref)) <= REF_TOL
    x = lm.log_grid()
    ref = lm.ref_log(x)
    assert _worst(mpmath, ref, [mpmath.log(mpmath.mpf(float(v))) for v in x], lm.ulp_of(ref)) <= REF_TOL
    x = lm.rcp_grid()
    ref = lm.ref_rcp(x)
    assert _worst(mpmath, ref, [1 / mpmath.mpf(float(v)) for v in x], lm.ulp_of(ref)) <= REF_TOL


def test_reference_logistic_agrees_with_mpmath(mpmath):
    """Every finite logit of the grid, with either response: w in ulps of w, g in ulps of 1, ll in ulps of max(|ll|, 1)
    -- the units of the device assertions.  (The transcendental part depends on |f| alone: computed once per |f|.)"""
    f, _ = lm.logistic_grid()
    af = np.unique(np.abs(_finite(f)))
    e = [mpmath.exp(-mpmath.mpf(float(v))) for v in af]
    l1p = [mpmath.log1p(t) for t in e]
    one = mpmath.mpf(1)
    for sign in (1.0, -1.0):
        for y in (0.0, 1.0):
            fs = sign * af
            ref = lm.ref_logistic(fs, np.full(fs.shape, y))
            w = [one + t for t in e]
            s = [(one / (one + t) if sign > 0 else t / (one + t)) for t in e]
            lin = [y * mpmath.mpf(float(v)) - max(mpmath.mpf(float(v)), 0) for v in fs]
            assert _worst(mpmath, ref['w'], w, lm.ulp_of(ref['w'])) <= REF_TOL
            assert _worst(mpmath, ref['g'], [y - t for t in s], np.full(fs.shape, 2.0 ** -52)) <= REF_TOL
            assert _worst(mpmath, ref['lin'], lin, lm.ulp_of_max1(ref['lin'])) <= REF_TOL
            assert _worst(mpmath, ref['ll'], [a - b for a, b in zip(lin, l1p)], lm.ulp_of_max1(ref['ll'])) <= REF_TOL


def test_reference_lse_and_p_right_agree_with_mpmath(mpmath):
    a, b = lm.lse_grid()
    ref = lm.ref_lse(a, b)
    ma, mb = [mpmath.mpf(float(v)) for v in a], [mpmath.mpf(float(v)) for v in b]
    exact = [max(p, q) + mpmath.log1p(mpmath.exp(-abs(p - q))) for p, q in zip(ma, mb)]
    assert _worst(mpmath, ref, exact, lm.ulp_of_max1(ref)) <= REF_TOL
    d = b - a
    ref = lm.ref_p_right(d)
    exact = [1 / (1 + mpmath.exp(-mpmath.mpf(float(v)))) for v in d]
    assert _worst(mpmath, ref, exact, lm.ulp_of(ref)) <= REF_TOL
