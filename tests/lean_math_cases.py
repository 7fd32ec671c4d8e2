"""Input grids and the long-double reference for the lean elementary functions of csrc/epx_device.h (rcp_d, exp_d,
log1p_unit_d, log_ge1_d, the logistic terms, log_sum_exp2 / merge_weights), shared by test_lean_math_cases.py (host: the
named edges are in the grids, the reference agrees with 50-digit arithmetic) and test_gpu_lean_math.py (device: the
functions themselves, through epx_math_probe).

The reference is np.longdouble: a 64-bit mantissa on x86, so its own error is about 2^-11 of a double ulp per operation.
Error is counted in ulps of the double nearest to the true result -- np.spacing, which is 2^-1074 for a subnormal
result, so that "units of 2^-1074" need no case of their own.  Not a test module: nothing here touches the device."""

import functools

import numpy as np

LD = np.longdouble
LN2 = float(np.log(2.0))
SQRT2_CUT = 1.4142135623730951           # log1p_unit_d folds m = 1 + e into [1/sqrt2, sqrt2] when m > this
INV_SQRT2_CUT = 0.70710678118654752      # log_ge1_d doubles the mantissa of frexp when it is below this
DBL_MIN, DBL_MAX = float(np.finfo(np.float64).tiny), float(np.finfo(np.float64).max)
SUB_UNIT = 5e-324                        # 2^-1074
FOLD = float((np.sqrt(LD(2)) - LD(1)).astype(np.float64))      # the double nearest to sqrt2 - 1


def _neighbours(v):
    v = np.atleast_1d(np.asarray(v, dtype=np.float64))
    return np.concatenate([np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)])


def holds(grid, v):
    """v is in the grid, bit for bit (so that -0.0 and NaN can be asked for)."""
    g = np.ascontiguousarray(grid, dtype=np.float64).view(np.uint64)
    if v != v:
        return bool(np.any(np.isnan(grid)))
    return bool(np.any(g == np.array([v], dtype=np.float64).view(np.uint64)[0]))


# ---------------------------------------------------------------------------------------------------------- grids
# The named edges of each grid: the host test asserts that every one of them is in the array the device test runs.
EXP_TO_ZERO = [-745.14, -746.0, -800.0, -801.0, -1e308, -np.inf]     # true result below 2^-1075: exactly 0
# exp(-745.13) = 0.5016 x 2^-1074: the correctly rounded result is 2^-1074, NOT 0 (ln 2^-1075 = -745.13322).  The point is
# in the grid as the last argument with a non-zero result and falls under the subnormal rule (1 unit of 2^-1074).
EXP_LAST_SUBNORMAL = [-745.13]
EXP_TO_INF = [709.79, 710.0, 800.0, 1e308, np.inf]
EXP_EDGES = [0.0, -0.0, 1e-300, -1e-300, np.nan] + EXP_TO_ZERO + EXP_LAST_SUBNORMAL + EXP_TO_INF
EXP_K = np.arange(-1000, 1001)


def exp_boundaries():
    """The rounding boundaries (k + 1/2) ln 2 of exp_d's range reduction, k = -1000 ... 1000, as doubles."""
    return (EXP_K + 0.5) * LN2


@functools.lru_cache(maxsize=None)
def exp_grid():
    rng = np.random.RandomState(1101)
    x = np.concatenate([rng.uniform(-40.0, 40.0, 20000), rng.uniform(-708.3, 709.7, 20000), rng.uniform(-0.35, 0.35, 20000),
                        _neighbours(exp_boundaries()), rng.uniform(-745.2, -708.3, 5000), np.array(EXP_EDGES)])
    x.setflags(write=False)
    return x


def log1p_branch_pair():
    """The largest e that log1p_unit_d does not fold (1 + e, rounded, is not above the cut) and the double after it."""
    e = np.nextafter(FOLD, -np.inf)
    while not (1.0 + np.nextafter(e, np.inf)) > SQRT2_CUT:
        e = np.nextafter(e, np.inf)
    return [float(e), float(np.nextafter(e, np.inf))]


LOG1P_EDGES = [0.0, 1.0, SUB_UNIT] + _neighbours(FOLD).tolist() + log1p_branch_pair()


@functools.lru_cache(maxsize=None)
def log1p_grid():
    rng = np.random.RandomState(1102)
    near = FOLD + rng.uniform(-1.0, 1.0, 2000) * 10.0 ** rng.uniform(-15.0, -2.0, 2000)
    e = np.concatenate([rng.uniform(0.0, 1.0, 30000), 10.0 ** rng.uniform(-300.0, 0.0, 5000), near, np.array(LOG1P_EDGES)])
    assert e.min() >= 0.0 and e.max() <= 1.0
    e.setflags(write=False)
    return e


LOG_EDGES = [1.0, DBL_MIN, DBL_MAX] + _neighbours(INV_SQRT2_CUT).tolist()
LOG_POS_EDGES = [0.0, -0.0]


@functools.lru_cache(maxsize=None)
def log_grid():
    """Positive, finite, NORMAL arguments (subnormal ones are outside the functions' stated domain)."""
    rng = np.random.RandomState(1103)
    x = np.concatenate([2.0 ** rng.uniform(-1020.0, 1020.0, 20000), rng.uniform(0.5, 2.0, 30000),
                        1.0 + rng.uniform(-1e-6, 1e-6, 3000), 2.0 ** rng.uniform(0.0, 300.0, 5000), np.array(LOG_EDGES)])
    assert x.min() >= DBL_MIN and np.all(np.isfinite(x))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def log_pos_grid():
    x = np.concatenate([log_grid(), np.array(LOG_POS_EDGES)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def rcp_grid():
    rng = np.random.RandomState(1104)
    x = np.concatenate([rng.uniform(1.0, 2.0, 30000), 2.0 ** rng.uniform(-1000.0, 1000.0, 10000)])
    x.setflags(write=False)
    return x


LOGISTIC_EXTRA = [36.0436, 37.0, 745.0, 800.0, 801.0, 1e4, 1e307]


@functools.lru_cache(maxsize=None)
def logistic_grid():
    """(f, y): the exp grid and its mirror image plus the saturation points of either sign, each with y = 0 and y = 1."""
    ex = np.array(LOGISTIC_EXTRA)
    f1 = np.concatenate([-exp_grid(), exp_grid(), ex, -ex])
    f = np.concatenate([f1, f1])
    y = np.concatenate([np.zeros(f1.shape[0]), np.ones(f1.shape[0])])
    f.setflags(write=False); y.setflags(write=False)
    return f, y


LSE_X = [-3.5, 0.0, 1e4]
# (a, b) -> what the plain definitions in the header return: log_sum_exp2[_lean], then merge_weights' (lse, p_right)
LSE_SPECIAL = ([((-np.inf, x), x, (x, 1.0)) for x in LSE_X] + [((x, -np.inf), x, (x, 0.0)) for x in LSE_X] +
               [((-np.inf, -np.inf), -np.inf, (-np.inf, np.nan)),
                ((np.inf, np.inf), np.inf, (np.nan, np.nan))])          # merge_weights forms exp(inf - inf)


@functools.lru_cache(maxsize=None)
def lse_grid():
    """(a, b): 10 000 finite pairs, a in [-1e4, 1e4] and a - b in [-800, 800]."""
    rng = np.random.RandomState(1105)
    a = rng.uniform(-1e4, 1e4, 10000)
    b = a - rng.uniform(-800.0, 800.0, 10000)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


# ---------------------------------------------------------------------------------------------------------- reference
def _quiet(fn):
    @functools.wraps(fn)
    def wrapped(*args):
        with np.errstate(all='ignore'):
            return fn(*args)
    return wrapped


@_quiet
def ref_exp(x):
    return np.exp(LD(1) * np.asarray(x))


@_quiet
def ref_rcp(x):
    return LD(1) / (LD(1) * np.asarray(x))


@_quiet
def ref_log1p(e):
    return np.log1p(LD(1) * np.asarray(e))


@_quiet
def ref_log(x):
    return np.log(LD(1) * np.asarray(x))


@_quiet
def ref_logistic(f, y):
    """The logistic terms written out in long double: w = 1 + exp(-|f|), g = y - sigmoid(f), lin = y f - max(f, 0),
    ll = lin - log(w).  (sigmoid through exp(-|f|), so that no intermediate overflows.)"""
    f, y = LD(1) * np.asarray(f), LD(1) * np.asarray(y)
    e = np.exp(-np.abs(f))
    w = LD(1) + e
    s = np.where(f >= 0, LD(1) / w, e / w)
    lin = y * f - np.maximum(f, LD(0))
    return {'w': w, 'g': y - s, 'lin': lin, 'll': lin - np.log1p(e)}


@_quiet
def ref_lse(a, b):
    a, b = LD(1) * np.asarray(a), LD(1) * np.asarray(b)
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    return hi + np.log1p(np.exp(lo - hi))


@_quiet
def ref_p_right(d):
    """e^b / (e^a + e^b) at the difference d = b - a."""
    d = LD(1) * np.asarray(d)
    e = np.exp(-np.abs(d))
    return np.where(d >= 0, LD(1) / (LD(1) + e), e / (LD(1) + e))


# ---------------------------------------------------------------------------------------------------------- error units
def ulp_of(ref):
    """Spacing of the doubles at the double nearest to `ref` (2^-1074 where that is subnormal or 0)."""
    with np.errstate(all='ignore'):
        return np.spacing(np.abs(np.asarray(ref).astype(np.float64)))


def ulp_of_max1(ref):
    with np.errstate(all='ignore'):
        return np.spacing(np.maximum(np.abs(np.asarray(ref).astype(np.float64)), 1.0))


def err_in(dev, ref, unit):
    """|dev - ref| / unit in long double."""
    with np.errstate(all='ignore'):
        return np.abs(LD(1) * np.asarray(dev) - ref) / (LD(1) * unit)


def err_ulps(dev, ref):
    return err_in(dev, ref, ulp_of(ref))
