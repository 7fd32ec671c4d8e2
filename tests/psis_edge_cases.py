"""The case table of the PSIS edge tests (plain helper, NumPy only, no tests): test_psis_edge_cases.py (no device) and
test_gpu_psis_edges.py (device) share it.

csrc/psis.h does not sort.  A bisection over the bit pattern of a threshold T looks for a count #{s : -lr_s < T} of
CANDIDATES within [M + 1, cand_cap(M)]; when one exists the candidates are listed and ranked among themselves (the
'listed' route), when ties keep every reachable count outside that window every draw is ranked against every draw (the
'all-pairs' route).  What decides the route and the sizes is written ONCE, here:

    M        = min(S // 5, ceil(3 sqrt(S)))            the tail; M < 5: nothing is smoothed ('short')
    tail_pad = M rounded up to even
    cand_cap = tail_pad + 16                           candidates the list holds
    m        = 30 + floor(sqrt(M))                     points of the Zhang-Stephens fit, at most FIT_MAX
    q        = floor(M / 4 + 0.5)                      the quartile x_q of the fit; x_q = 0: not smoothed
    scratch  = tail_pad + cand_cap + cand_cap / 2 + FIT_MAX + 2   doubles per row, 16 rows per workgroup

A tie cluster with `inside` members in the tail and `below` under it has the reachable counts 1 .. M - inside, then
M + below: it is listed exactly when M + below <= cand_cap(M), that is below <= 16 for even M and <= 17 for odd M.

Every family is a function of (S, seed) and states the route and whether the row is smoothed as it EXPECTS them, from M
alone; the CPU test holds that against route() -- the rule above on the sorted row -- and against loo.psis_host.  The
KHAT each smoothed case expects is the interval +-KHAT_HALF_WIDTH about the value recorded in
tests/golden/psis_edge_khat.txt (the float64 host statement at that seed; `python tests/psis_edge_cases.py` writes it).
A case at which the float64 and the longdouble statement part on smoothed / not smoothed gets another seed (SEEDS), never
an exemption."""

import math
import os

import numpy as np

MIN_TAIL, FIT_MAX = 5, 64               # csrc/psis.h: PSIS_MIN_TAIL, PSIS_FIT_MAX
ROWS_PER_GROUP = 16                     # rows of a workgroup of k_psis_rows, each with its own scratch
LDS_RESERVE = 1024                      # epx_psis_rows: lds > capacity - 1024 is refused
KHAT_HALF_WIDTH = 0.5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'psis_edge_khat.txt')


# ---------------------------------------------------------------- the sizes
def tail_length(S):
    c = math.isqrt(9 * S)
    return min(S // 5, c if c * c == 9 * S else c + 1)


def tail_pad(M):
    return (M + 1) // 2 * 2


def cand_cap(M):
    return tail_pad(M) + 16


def fit_points(M):
    return 30 + math.isqrt(M)


def quartile(M):
    return int(math.floor(M / 4 + 0.5))


def scratch_doubles(M):
    return tail_pad(M) + cand_cap(M) + cand_cap(M) // 2 + FIT_MAX + 2


def lds_bytes(M):
    return ROWS_PER_GROUP * scratch_doubles(M) * 8


def served(S, capacity):
    """Whether epx_psis_rows takes S draws per row at an LDS of `capacity` bytes."""
    M = tail_length(S)
    return fit_points(M) <= FIT_MAX and lds_bytes(M) <= capacity - LDS_RESERVE


# what tests/psis_plan_probe.hip must find (asserted against it, never used instead of it)
S_MAX = 24753                           # M = 472: the last S served; S_MAX + 1 has M = 473 and is refused


# ---------------------------------------------------------------- the route
def route(ll):
    """'short', 'listed' or 'all-pairs' for ONE row: listed when some T gives a count #{s : -lr_s < T} within
    [M + 1, cand_cap(M)].  With a = -lr ascending the reachable counts are the i with a[i - 1] < a[i], and S."""
    ll = np.asarray(ll, dtype=np.float64)
    S = ll.shape[0]
    M = tail_length(S)
    if M < MIN_TAIL:
        return 'short'
    if S <= cand_cap(M):
        return 'listed'
    a = np.sort(-(-ll - (-ll).max()))
    reach = set((np.nonzero(a[1:] > a[:-1])[0] + 1).tolist()) | {S}
    return 'listed' if any(M + 1 <= n <= cand_cap(M) for n in reach) else 'all-pairs'


# ---------------------------------------------------------------- the families
def gauss(S, seed):
    """The first Gaussian row of test_gpu_loo._psis_inputs(S, seed)."""
    th = 0.2 + 0.5 * np.random.RandomState(1000 * seed).randn(S)
    return -0.5 * np.log(2 * np.pi) - 0.5 * np.square(0.7 - th)


def bern(S, seed):
    """The first Bernoulli row (y = 0) of test_gpu_loo._psis_inputs(S, seed)."""
    f = 3.0 * np.random.RandomState(seed).randn(S)
    return 0.0 * f - (np.maximum(f, 0.0) + np.log1p(np.exp(-np.abs(f))))


def pareto(k):
    def row(S, seed):
        return -k * np.random.RandomState(seed + 7).exponential(size=S)
    return row


def uniform(S, seed):
    return -np.log(np.random.RandomState(seed + 11).uniform(1.0, 2.0, size=S))


def _by_ratio(ll):
    """The draws in ascending order of (lr, s): the last M are the tail."""
    return np.argsort(-ll, kind='stable')


def cluster(below, inside):
    """The gauss row with the draws of rank S - M - below .. S - M + inside - 1 (ascending ratio) set to one value, then
    permuted (the ranks are cut at 0 and S - 1)."""
    def row(S, seed):
        ll = gauss(S, seed)
        M = tail_length(S)
        order = _by_ratio(ll)
        lo, hi = max(0, S - M - below), min(S - 1, S - M + inside - 1)
        ll[order[lo:hi + 1]] = ll[order[S - M - 1]]
        return ll[np.random.RandomState(seed + 13).permutation(S)]
    return row


def twice(S, seed):
    """Every draw occurs twice (S odd: but the one of the smallest ratio), permuted."""
    base = gauss((S + 1) // 2, seed)
    base = base[_by_ratio(base)]
    ll = np.concatenate([base, base[S % 2:]])
    return ll[np.random.RandomState(seed + 17).permutation(S)]


def top_tied(count):
    """The `count(M)` largest ratios tied."""
    def row(S, seed):
        ll = gauss(S, seed)
        order = _by_ratio(ll)
        n = min(S, count(tail_length(S)))
        ll[order[S - n:]] = ll[order[S - n]]
        return ll[np.random.RandomState(seed + 19).permutation(S)]
    return row


def scale(f):
    return lambda S, seed: f * gauss(S, seed)


def offset(v):
    return lambda S, seed: gauss(S, seed) + v


def constant(S, seed):
    return np.full(S, -0.3)


def level_counts(S):
    n1, n2 = (3 * S) // 5, (3 * S) // 10
    return n1, n2, S - n1 - n2


def levels(S, seed):
    """test_gpu_loo._tied: three tied levels, 60 % / 30 % / 10 % of the draws; the 10 % hold the largest ratio."""
    n1, n2, n3 = level_counts(S)
    return np.concatenate([np.full(n1, -0.1), np.full(n2, -0.2), np.full(n3, -3.0)])


def far_below(S, seed):
    """The counter-example kept OUT of the device table: one draw's ll 800 below the rest, so every other ratio is
    exp(-800) of the largest.  exp(lr) underflows to 0 in float64 (all excesses but the top one 0: not smoothed);
    longdouble holds it and smooths.  This is why the table demands that the two statements agree on the pattern."""
    ll = gauss(S, seed)
    ll[np.argmin(ll)] -= 800.0
    return ll


# ---------------------------------------------------------------- what every family expects, from M alone
def _listed_iff(n, M):
    return 'listed' if M + 1 <= n <= cand_cap(M) else 'all-pairs'


def _cluster_expect(below, inside):
    # reachable counts: 1 .. M - inside, then M + below (S >= 25: M + below <= S, and S itself is beyond the cap);
    # `inside` tail members tie with u, their excess is 0: smoothed when x_q is not one of them
    return lambda S, M: (_listed_iff(M + min(below, S - M), M), inside < quartile(M))


def _levels_route(S, M):
    n1, n2, n3 = level_counts(S)
    return 'listed' if 'listed' in (_listed_iff(n3, M), _listed_iff(n3 + n2, M)) else 'all-pairs'


class Family:
    def __init__(self, name, row, expect):
        self.name, self.row, self.expect = name, row, expect


_continuous = lambda S, M: ('listed', True)
FAMILIES = [
    Family('gauss', gauss, _continuous),
    Family('bern', bern, _continuous),
    Family('pareto0.3', pareto(0.3), _continuous),
    Family('pareto0.7', pareto(0.7), _continuous),
    Family('pareto1.2', pareto(1.2), _continuous),
    Family('pareto3', pareto(3.0), _continuous),
    Family('uniform', uniform, _continuous),
    Family('cluster30.2', cluster(30, 2), _cluster_expect(30, 2)),          # all-pairs, smoothed from q = 3 on
    Family('cluster40.0', cluster(40, 0), lambda S, M: ('all-pairs', True)),
    Family('cluster5.1', cluster(5, 1), _cluster_expect(5, 1)),             # listed, a tie across the tail's boundary
    Family('cluster16.1', cluster(16, 1), lambda S, M: ('listed', quartile(M) > 1)),
    Family('cluster17.1', cluster(17, 1), lambda S, M: ('listed' if M % 2 else 'all-pairs', quartile(M) > 1)),
    Family('cluster18.1', cluster(18, 1), lambda S, M: ('all-pairs', quartile(M) > 1)),
    Family('cluster8.8', cluster(8, 8), lambda S, M: ('listed', quartile(M) > 8)),
    # pairs: an odd tail splits a pair with u, one excess is 0
    Family('twice', twice, lambda S, M: ('listed', M % 2 < quartile(M))),
    Family('top3', top_tied(lambda M: 3), _continuous),
    Family('top_many', top_tied(lambda M: M + 20), lambda S, M: ('all-pairs', False)),
    Family('scale1e-6', scale(1e-6), _continuous),
    Family('offset1e8', offset(1e8), _continuous),
    Family('scale1e-300', scale(1e-300), lambda S, M: ('listed', False)),   # every exp(lr) is 1
    Family('constant', constant, lambda S, M: ('all-pairs', False)),
    # counts n3, n3 + n2, S; the tail's top n3 excesses are equal and the rest 0 (or all of them 0): x_M > x_q > 0 fails
    Family('levels', levels, lambda S, M: (_levels_route(S, M), False)),
]
BY_NAME = dict((f.name, f) for f in FAMILIES)

# every S from 25 to 130 (M = 5 .. 26, both parities, m = 32 .. 35); 180: M = 36 through S / 5; 225 | 226: the two arms
# of M cross; 246, 266, 267: M = 48, 49, 50 (C around 64, m changes); 400, 441: M = 60, 63 (C crosses 64); 455: M = 64
S_LIST = list(range(25, 131)) + [180, 225, 226, 246, 266, 267, 400, 441, 455, 2000]
S_CLAIMS = {25: 5, 130: 26, 180: 36, 225: 45, 226: 45, 246: 48, 266: 49, 267: 50, 400: 60, 441: 63, 455: 64, 2000: 135}

# (family, S) -> seed, where the default seed S makes the float64 and the longdouble statement part
SEEDS = {}


class Case:
    def __init__(self, family, S):
        self.family, self.S, self.M = family.name, S, tail_length(S)
        self.seed = SEEDS.get((family.name, S), S)
        self.route, self.smoothed = family.expect(S, self.M)
        self.id = '%s-S%d' % (family.name, S)
        self._row = family.row

    def ll(self):
        return np.ascontiguousarray(self._row(self.S, self.seed), dtype=np.float64)

    def __repr__(self):
        return self.id


def cases(S):
    return [Case(f, S) for f in FAMILIES]


def rows(S):
    """All case rows of one S, stacked (n, S), in the order of FAMILIES."""
    return np.ascontiguousarray(np.stack([c.ll() for c in cases(S)]))


def case(name, S):
    return Case(BY_NAME[name], S)


LIMIT_FAMILIES = ['gauss'] * 4 + ['pareto1.2'] * 2 + ['cluster40.0']      # the rows at S_MAX (and one past it)


def limit_rows(S):
    return np.ascontiguousarray(np.stack([BY_NAME[name].row(S, S + i) for i, name in enumerate(LIMIT_FAMILIES)]))


def khat_table():
    """{(family, S): the recorded KHAT} of the smoothed cases (tests/golden/psis_edge_khat.txt)."""
    out = {}
    with open(GOLDEN) as f:
        for line in f:
            if line.strip() and not line.startswith('#'):
                name, S, k = line.split()
                out[(name, int(S))] = float(k)
    return out


def _write_golden():
    from epstan_amd import loo
    with open(GOLDEN, 'w') as f:
        f.write('# family S KHAT: loo.psis_host (float64) on every smoothed case of tests/psis_edge_cases.py\n')
        for S in S_LIST:
            for c in cases(S):
                k = float(loo.psis_host(c.ll()[None, :])[0, 1])
                if np.isfinite(k):
                    f.write('%s %d %.6f\n' % (c.family, S, k))


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _write_golden()
