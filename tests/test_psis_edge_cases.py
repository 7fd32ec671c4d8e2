"""(no device) The case table of the PSIS edge tests, psis_edge_cases.py, against the host statement loo.psis_host and
the library's own size functions.

 * Routes: the rule route() gives every case the route its family expects from M alone, every case is smoothed or not
   as it expects, and every S has a smoothed row on each route: the device test then compares csrc/psis.h with the host
   on routes that are known to be taken.
 * Agreement: the float64 and the longdouble statement agree on smoothed / not smoothed in every case.  That is a
   condition on the table (a case that breaks it gets another seed), so that a device result that parts from the host
   in the pattern has no rounding to plead.  One counter-example is asserted here and kept out of the device table.
 * The yardstick: on the smoothed cases of S = 25, 50, 100 a 40-digit mpmath restatement of loo._psis_row lies within
   max(|float64 - longdouble| / 16, 2^-60 |value|) of the longdouble result: |float64 - longdouble| measures the float64
   statement's own error, which the device test's bound is a multiple of.
 * Sizes: the restatements of psis_edge_cases.py equal csrc/psis.h's functions (tests/psis_plan_probe.hip, linked with
   libepx.so) at every S of the list, and the largest S epx_psis_rows serves comes out of the probe."""

import math
import subprocess

import numpy as np
import pytest

import psis_edge_cases as pc
from epstan_amd import loo
from test_tree_endings_cases import _build_probe

_host = {}


def _results(S):
    """(ll, float64 result, longdouble result) of all case rows of one S, computed once."""
    if S not in _host:
        ll = pc.rows(S)
        with np.errstate(all='ignore'):
            wide = loo.psis_host(ll.astype(np.longdouble))
        _host[S] = (ll, loo.psis_host(ll), wide)
    return _host[S]


# ------------------------------------------------------------------ routes and patterns
def test_the_s_list_is_the_one_stated():
    assert len(pc.S_LIST) == 116 == len(set(pc.S_LIST))
    for S, M in pc.S_CLAIMS.items():
        assert S in pc.S_LIST and pc.tail_length(S) == M == loo.tail_length(S), S
    Ms = set(pc.tail_length(S) for S in range(25, 131))
    assert Ms == set(range(5, 27))
    assert set(pc.fit_points(M) for M in Ms) == {32, 33, 34, 35}
    assert [pc.fit_points(M) for M in (8, 9, 15, 16, 24, 25, 35, 36, 48, 49, 63, 64)] == [32, 33, 33, 34, 34, 35, 35, 36, 36, 37,
                                                                                    37, 38]
    assert [pc.quartile(M) for M in (5, 6, 9, 10, 13, 14, 33, 34)] == [1, 2, 2, 3, 3, 4, 8, 9]
    # C = M + 1 .. cand_cap(M) candidates: one block of 64 up to M = 46, either below M = 64, two from there on
    assert pc.cand_cap(46) == 62 and pc.cand_cap(48) == 64 and pc.cand_cap(49) == 66
    assert all(pc.tail_length(S) + 1 <= 64 < pc.cand_cap(pc.tail_length(S)) for S in (266, 267, 400, 441))
    assert pc.tail_length(455) + 1 > 64


def test_the_first_rows_are_those_of_the_existing_test():
    from test_gpu_loo import _psis_inputs, _tied
    for S in (25, 50, 226):
        ref = _psis_inputs(S, S)
        assert np.array_equal(pc.gauss(S, S), ref[0]) and np.array_equal(pc.bern(S, S), ref[17])
        assert np.array_equal(pc.constant(S, S), ref[35]) and np.array_equal(pc.levels(S, S), ref[36])
        assert np.array_equal(pc.levels(S, S), _tied(S))


@pytest.mark.parametrize('S', pc.S_LIST)
def test_every_case_takes_the_route_and_has_the_pattern_it_expects(S):
    ll, host, wide = _results(S)
    khat = pc.khat_table()
    seen = set()
    for i, c in enumerate(pc.cases(S)):
        assert np.all(np.isfinite(ll[i])) and ll[i].shape == (S,)
        assert pc.route(ll[i]) == c.route, (c, c.M, pc.route(ll[i]))
        assert bool(np.isfinite(host[i, 1])) == c.smoothed, (c, c.M, host[i])
        # the two statements agree on the pattern: a condition on the table
        assert bool(np.isfinite(float(wide[i, 1]))) == c.smoothed, (c, c.M, wide[i])
        assert np.isfinite(host[i, 0]) and np.isfinite(host[i, 2])
        if c.smoothed:
            seen.add(c.route)
            assert abs(host[i, 1] - khat[(c.family, S)]) <= pc.KHAT_HALF_WIDTH, (c, host[i, 1])
        else:
            assert (c.family, S) not in khat and np.isposinf(host[i, 1])
    assert seen == {'listed', 'all-pairs'}, (S, seen)          # a smoothed row on each route at every S


def test_the_rows_at_the_size_limit():
    ll = pc.limit_rows(pc.S_MAX)
    assert ll.shape == (7, pc.S_MAX) and pc.tail_length(pc.S_MAX) == 472
    assert [pc.route(r) for r in ll] == ['listed'] * 6 + ['all-pairs']
    host = loo.psis_host(ll)
    with np.errstate(all='ignore'):
        wide = loo.psis_host(ll.astype(np.longdouble))
    assert np.all(np.isfinite(host)) and np.all(np.isfinite(wide.astype(np.float64)))
    assert len(set(host[:, 1].tolist())) == 7 and host[4:6, 1].min() > 0.7 > host[:4, 1].max()


def test_the_table_spans_the_fit():
    k = np.array(list(pc.khat_table().values()))
    assert k.min() < -0.9 and k.max() > 3.0                      # bounded ratios to a tail without a mean
    assert len(k) == sum(c.smoothed for S in pc.S_LIST for c in pc.cases(S))


def test_the_route_switch_sits_where_the_formula_says():
    """A cluster of `below` draws under the tail and `inside` in it is listed iff M + below <= cand_cap(M)."""
    evens = [S for S in pc.S_LIST if pc.tail_length(S) % 2 == 0]
    odds = [S for S in pc.S_LIST if pc.tail_length(S) % 2 == 1]
    assert len(evens) > 40 and len(odds) > 40
    for S in evens + odds:
        M = pc.tail_length(S)
        for below in (16, 17, 18):
            want = 'listed' if M + below <= pc.cand_cap(M) else 'all-pairs'
            assert pc.route(pc.case('cluster%d.1' % below, S).ll()) == want, (S, below)
    # literally: S = 50 (M = 10, 26 candidates at most), S = 55 (M = 11, 28 at most)
    assert (pc.tail_length(50), pc.cand_cap(10), pc.tail_length(55), pc.cand_cap(11)) == (10, 26, 11, 28)
    assert [pc.route(pc.case('cluster%d.1' % b, 50).ll()) for b in (16, 17, 18)] == ['listed', 'all-pairs', 'all-pairs']
    assert [pc.route(pc.case('cluster%d.1' % b, 55).ll()) for b in (16, 17, 18)] == ['listed', 'listed', 'all-pairs']
    # and the cluster is where its name says: `below + inside` equal values, `inside` of them in the tail
    for name, below, inside in (('cluster16.1', 16, 1), ('cluster30.2', 30, 2), ('cluster40.0', 40, 0), ('cluster5.1', 5, 1)):
        ll = pc.case(name, 400).ll()
        a = np.sort(-ll)                                           # ascending ratio
        M = pc.tail_length(400)
        tied = np.nonzero(a == a[400 - M - 1])[0]
        assert tied.tolist() == list(range(400 - M - below, 400 - M + inside)), name


def test_short_and_trivially_listed_rows():
    assert pc.route(np.zeros(24)) == 'short' and pc.route(np.zeros(25)) == 'all-pairs'
    assert pc.route(np.arange(25.0)) == 'listed'


def test_rows_with_duplicates_are_what_they_say():
    for S in (50, 51, 226):
        v, n = np.unique(pc.twice(S, S), return_counts=True)
        assert sorted(n.tolist()) == [1] * (S % 2) + [2] * (S // 2)
        if S % 2:
            assert v[n == 1][0] == v.max()                         # the single draw has the smallest ratio
        M = pc.tail_length(S)
        top = np.sort(pc.case('top3', S).ll())
        assert top[0] == top[2] < top[3]
        many = np.sort(pc.case('top_many', S).ll())
        assert many[0] == many[M + 19] < many[M + 20]


def test_a_pattern_the_two_statements_part_on():
    """One draw 800 below the rest: exp(lr) of every other draw underflows in float64 and all excesses but the largest are
    0, so the row is not smoothed; longdouble keeps exp(-800) and smooths.  Such a row cannot be held against the host by
    a bound derived from |float64 - longdouble|, which is why the device table admits none."""
    ll = pc.far_below(50, 50)[None, :]
    assert pc.route(ll[0]) == 'listed'
    assert np.isposinf(loo.psis_host(ll)[0, 1])
    with np.errstate(all='ignore'):
        assert np.isfinite(float(loo.psis_host(ll.astype(np.longdouble))[0, 1]))


# ------------------------------------------------------------------ the longdouble yardstick
def _psis_row_mp(ll):
    """loo._psis_row on a smoothed row, restated in 40-digit mpmath arithmetic (ll: float64)."""
    import mpmath as mp
    mp.mp.dps = 40
    S = len(ll)
    M = loo.tail_length(S)
    v = [mp.mpf(float(x)) for x in ll]
    top = max(-x for x in v)
    lr = [-x - top for x in v]
    order = sorted(range(S), key=lambda s: (lr[s], s))
    tail = order[S - M:]
    eu = mp.exp(lr[order[S - M - 1]])
    x = [mp.exp(lr[s]) - eu for s in tail]
    m = 30 + math.isqrt(M)
    xq = x[int(math.floor(M / 4 + 0.5)) - 1]
    assert xq > 0 and x[-1] > xq
    b = [1 / x[-1] + (1 - mp.sqrt(mp.mpf(m) / (i - mp.mpf(0.5)))) / (3 * xq) for i in range(1, m + 1)]
    k = [sum(mp.log1p(-bi * xj) for xj in x) / M for bi in b]
    L = [M * (mp.log(-bi / ki) - ki - 1) for bi, ki in zip(b, k)]
    w = [1 / sum(mp.exp(Lj - Li) for Lj in L) for Li in L]
    bb = sum(bi * wi for bi, wi in zip(b, w))
    kk = sum(mp.log1p(-bb * xj) for xj in x) / M
    sigma = -kk / bb
    khat = (M * kk + 5) / (M + 10)
    for j, s in enumerate(tail):
        p = (mp.mpf(j + 1) - mp.mpf(0.5)) / M
        q = (sigma / khat) * mp.expm1(-khat * mp.log1p(-p))
        lr[s] = min(mp.mpf(0), mp.log(eu + q))

    def lse(t):
        big = max(t)
        return big + mp.log(sum(mp.exp(a - big) for a in t))
    norm = lse(lr)
    lw = [a - norm for a in lr]
    return lse([a + c for a, c in zip(lw, v)]), khat, 1 / sum(mp.exp(2 * a) for a in lw)


@pytest.mark.parametrize('S', [25, 50, 100])
def test_the_longdouble_statement_is_a_valid_yardstick(S):
    import mpmath as mp
    ll, host, wide = _results(S)
    n = 0
    for i, c in enumerate(pc.cases(S)):
        if not c.smoothed:
            continue
        n += 1
        exact = _psis_row_mp(ll[i])
        for col in range(3):
            hi = float(wide[i, col])                                # (a longdouble is the exact sum of two doubles)
            w = mp.mpf(hi) + mp.mpf(float(wide[i, col] - np.longdouble(hi)))
            span = abs(float(host[i, col]) - w)
            assert abs(w - exact[col]) <= max(span / 16, mp.mpf(2) ** -60 * abs(exact[col])), (c, col, float(span),
                                                                                                 float(abs(w - exact[col])))
    assert n >= 11                                                # (S = 25: q = 1, a single tie with u leaves a row as it is)


# ------------------------------------------------------------------ the sizes
def test_sizes_are_the_librarys(tmp_path):
    exe = _build_probe(tmp_path, 'psis_plan_probe')
    capacity, min_tail, fit_max = (int(w) for w in subprocess.check_output([exe, 'cap']).decode().split())
    assert (min_tail, fit_max) == (pc.MIN_TAIL, pc.FIT_MAX) and capacity == 160 * 1024
    sweep = sorted(set(pc.S_LIST) | set(range(1, 25)) | {pc.S_MAX - 1, pc.S_MAX, pc.S_MAX + 1, 100000})
    out = subprocess.check_output([exe, 'sizes'] + [str(S) for S in sweep]).decode().splitlines()
    assert len(out) == len(sweep)
    for S, line in zip(sweep, out):
        M = pc.tail_length(S)
        want = [S, M, pc.fit_points(M), pc.tail_pad(M), pc.cand_cap(M), pc.scratch_doubles(M)]
        assert [int(w) for w in line.split()] == want, (line, want)
        assert pc.lds_bytes(M) == 16 * 8 * want[5]
    first, last = ([int(w) for w in line.split()] for line in subprocess.check_output([exe, 'first']).decode().splitlines())
    assert (last[0], first[0]) == (pc.S_MAX, pc.S_MAX + 1)
    assert (last[1], first[1]) == (472, 473)
    assert pc.served(pc.S_MAX, capacity) and not pc.served(pc.S_MAX + 1, capacity)
    assert first[2] <= fit_max                                    # (the LDS, not the fit length, is what refuses first)
    assert 16 * 8 * last[5] <= capacity - 1024 < 16 * 8 * first[5]
