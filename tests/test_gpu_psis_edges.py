"""csrc/psis.h on the device at the edges the case table tests/psis_edge_cases.py names: tied tails on both order routes,
the switch between the routes, every lane-level edge of the sizes, heavy and bounded tails, the rows of a wave under
divergence, the LDS limit, and the two other consumers (k_loo, k_reweight) on duplicated draws.  Need a real MI355X.

test_psis_edge_cases.py (no device) shows that every case takes the route it expects and that the float64 and the
longdouble host statement agree on which rows are smoothed; here the device is held against loo.psis_host.

The bound is test_gpu_loo._psis_check's, unchanged: the device may differ from the float64 host by 100 x the largest
|float64 - longdouble| of the host statement over the rows of a call, floored at 1e-12 relative; the smoothed pattern
must agree exactly.  A call stacks all families of one S, and two of them (ll + 1e8 in ELPD, ll x 1e-6 in KHAT) have a
spread orders above the others', so beside the call's check every case is ASSERTED against the bound of ITS OWN row: the
same expression with the row's own |float64 - longdouble|.

Nothing on the device tells which route a row took: that the cases take the routes they state rests on
psis_edge_cases.route() restating the bisection of psis_smooth (the count #{-lr_s < T} is monotone in T and the
bisection lands exactly when some reachable count lies in [M + 1, psis_cand_cap(M)]).  Whoever changes that bisection
changes route() with it.

Measured on an MI355X (sections 3.2 and 5): 2 552 cases, 1 857 listed and 695 all-pairs, 1 932 smoothed with KHAT
-0.995 .. 3.496; largest error / bound of a call 0.34 (the ll x 1e-6 family at S = 90, whose excesses cancel seven digits;
every other family below 3.3e-2 of its own row's bound), 2.6e-2 at S = 24 753; the file's 130 tests take 5.6 s.

EPX_PSIS_MARGINS=<file>: the figures of the run are written there (profiles/psis_edges_margins.txt is such a file)."""

import itertools
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import psis_edge_cases as pc                                    # noqa: E402
from epstan_amd import _lib, loo                                # noqa: E402
from epstan_amd.engine import HipEngine, MODEL_IDS, is_gauss    # noqa: E402
from test_gpu_parity import _site_problem                       # noqa: E402
from test_gpu_loo import _psis_check, _assert_loo_site, _rows_problem, PSIS_NAMES      # noqa: E402
from test_gpu_reweight import Case, check_against_host, same_bytes                    # noqa: E402

KHAT_EXPECTED = pc.khat_table()
RECORD = {'A': {}, 'C': [], 'D': [], 'routes': {}, 'khat': [np.inf, -np.inf], 'worst': 0.0}


@pytest.fixture(scope='module')
def eng():
    X, y, k_lim, _, _, _, _ = _site_problem('m1b_sg', 2, 7, 5, K=2)
    e = HipEngine('m1b_sg', X, y, k_lim)
    yield e
    e.close()


@pytest.fixture(scope='module', autouse=True)
def _margins_file():
    yield
    path = os.environ.get('EPX_PSIS_MARGINS')
    if not path or not RECORD['A']:
        return
    fams = [f.name for f in pc.FAMILIES]
    with open(path, 'w') as f:
        f.write('# tests/test_gpu_psis_edges.py: largest error / bound, the bound of test_gpu_loo._psis_check (100 x |float64 -\n'
                '# longdouble| of loo.psis_host, floored at 1e-12 relative).  "call": over the rows of the call, as asserted;\n'
                '# "own": each row against the bound of its own row, also asserted (per S the largest, with its family and\n'
                '# column; per family the largest over all S, ELPD KHAT WESS).\n')
        f.write('# no case has a widened bound\n')
        f.write('# cases by route (all S): %s; smoothed: %s\n' % (
            ', '.join('%s %d' % kv for kv in sorted(RECORD['routes'].items())), RECORD.get('smoothed', 0)))
        f.write('# KHAT of the smoothed cases on the device: %.3f .. %.3f\n' % tuple(RECORD['khat']))
        f.write('# largest error / bound over all calls: %.3e\n' % RECORD['worst'])
        for line in RECORD['C'] + RECORD['D']:
            f.write('# %s\n' % line)
        worst = dict((name, [0.0, 0.0, 0.0]) for name in fams)
        for S in sorted(RECORD['A']):
            call, rows = RECORD['A'][S]
            top = max(((v or 0.0, name, PSIS_NAMES[c]) for name, route, r in rows for c, v in enumerate(r)))
            f.write('S=%d M=%d call %.2e own %.2e %s %s\n' % ((S, pc.tail_length(S), call) + top))
            for name, route, r in rows:
                worst[name] = [max(a, b or 0.0) for a, b in zip(worst[name], r)]
        f.write('largest over all S, per family (own-row bound):\n')
        for name in fams:
            f.write('  %-12s %s\n' % (name, ' '.join('%.2e' % v for v in worst[name])))


def _own_row_ratios(got, ll):
    """Every row's |device - host| over the bound of that row alone: [(ELPD, KHAT, WESS)]; None where the row has no such
    figure (KHAT of a row that is not smoothed; an exact 0 with no spread has no scale of its own: the call's bound)."""
    host = loo.psis_host(ll)
    with np.errstate(all='ignore'):
        wide = loo.psis_host(ll.astype(np.longdouble))
    out = []
    for i in range(len(ll)):
        r = []
        for c in range(3):
            if c == 1 and np.isinf(host[i, 1]):
                r.append(None)
                continue
            ref = abs(float(host[i, c] - wide[i, c]))
            err, bound = abs(got[i, c] - host[i, c]), max(100.0 * ref, 1e-12 * abs(host[i, c]))
            r.append(err / bound if bound > 0.0 else None)
        out.append(tuple(r))
    return out


# ------------------------------------------------------------------ A. parity, every S of the list
_part_a = {}


def _device_rows(eng, S):
    if S not in _part_a:
        _part_a[S] = eng.psis_rows(pc.rows(S))
    return _part_a[S]


@pytest.mark.parametrize('S', pc.S_LIST)
def test_every_case_matches_the_host(eng, S):
    ll = pc.rows(S)
    cases = pc.cases(S)
    got = _device_rows(eng, S)
    assert got.shape == (len(cases), 3)
    assert got.tobytes() == eng.psis_rows(ll).tobytes()                 # twice: the same bytes
    smoothed = np.array([c.smoothed for c in cases])
    assert np.array_equal(np.isfinite(got[:, 1]), smoothed), [c for c, g in zip(cases, got) if np.isfinite(g[1]) != c.smoothed]
    call = _psis_check(got, ll, 'S=%d' % S)
    khat = KHAT_EXPECTED
    rows = []
    for c, g, r in zip(cases, got, _own_row_ratios(got, ll)):
        rows.append((c.family, c.route, r))
        assert all(v is None or v <= 1.0 for v in r), (c, dict(zip(PSIS_NAMES, r)), g)      # the bound of its own row
        RECORD['routes'][c.route] = RECORD['routes'].get(c.route, 0) + 1
        if c.smoothed:
            assert abs(g[1] - khat[(c.family, S)]) <= pc.KHAT_HALF_WIDTH, (c, g)
            RECORD['khat'] = [min(RECORD['khat'][0], g[1]), max(RECORD['khat'][1], g[1])]
            RECORD['smoothed'] = RECORD.get('smoothed', 0) + 1
        else:
            # not smoothed: the plain self-normalised estimate, whatever the route made of the ranks
            w = np.exp(-c.ll() - (-c.ll()).max())
            np.testing.assert_allclose(g[2], w.sum() ** 2 / np.square(w).sum(), rtol=1e-11)
    RECORD['A'][S] = (call, rows)
    RECORD['worst'] = max(RECORD['worst'], call)
    print('S=%d: largest error / bound of the call %.3e' % (S, call))


# ------------------------------------------------------------------ B. the rows of a wave are independent
def _four_kinds(S):
    """A listed smoothed row, an all-pairs smoothed one, an all-pairs row that is not smoothed, and one with a NaN."""
    kinds = [pc.case('gauss', S), pc.case('cluster40.0', S), pc.case('top_many', S)]
    assert [(c.route, c.smoothed) for c in kinds] == [('listed', True), ('all-pairs', True), ('all-pairs', False)]
    bad = pc.case('pareto0.7', S).ll()
    bad[S // 3] = np.nan
    return [c.ll() for c in kinds] + [bad]


def _alone(eng, row):
    return eng.psis_rows(row[None, :])[0].tobytes()


@pytest.mark.parametrize('S', [50, 400])
def test_four_kinds_of_rows_in_every_order(eng, S):
    rows = _four_kinds(S)
    alone = [_alone(eng, r) for r in rows]
    first = np.frombuffer(b''.join(alone), dtype=np.float64).reshape(4, 3)
    assert np.all(np.isfinite(first[:2])) and np.isposinf(first[2, 1]) and np.all(np.isnan(first[3]))
    assert len(set(alone)) == 4
    for order in itertools.permutations(range(4)):
        got = eng.psis_rows(np.stack([rows[i] for i in order]))
        for at, i in enumerate(order):
            assert got[at].tobytes() == alone[i], (S, order, at)


@pytest.mark.parametrize('S', [50, 400])
def test_a_row_gives_its_bytes_at_every_place_and_count(eng, S):
    rows = _four_kinds(S)
    tied = pc.case('cluster5.1', S)                                   # and a listed row with a tie across the tail's boundary
    assert (tied.route, tied.smoothed) == ('listed', True)
    rows.append(tied.ll())
    fill = np.stack([pc.gauss(S, 100 + i) for i in range(20)])
    assert all(pc.route(r) == 'listed' for r in fill)
    fill_alone = [_alone(eng, r) for r in fill]
    for kind in (1, 2, 3, 4):                                         # another DPP row, wave and workgroup: 0 .. 19
        own = _alone(eng, rows[kind])
        for at in range(20):
            ll = fill.copy()
            ll[at] = rows[kind]
            got = eng.psis_rows(ll)
            assert got[at].tobytes() == own, (S, kind, at)
            assert all(got[i].tobytes() == fill_alone[i] for i in range(20) if i != at), (S, kind, at)
    mixed = np.stack([rows[(i + 1) % 4] for i in range(17)])        # the partial last wave, the second workgroup
    alone = [_alone(eng, r) for r in rows]
    for n in (1, 3, 4, 5, 16, 17):
        got = eng.psis_rows(mixed[:n])
        assert all(got[i].tobytes() == alone[(i + 1) % 4] for i in range(n)), (S, n)


# ------------------------------------------------------------------ C. the LDS limit
def test_the_largest_s_is_served_and_the_next_refused(eng):
    S = pc.S_MAX
    assert pc.tail_length(S) == 472 and pc.tail_length(S + 1) == 473
    ll = pc.limit_rows(S)
    assert [pc.route(r) for r in ll] == ['listed'] * 6 + ['all-pairs']
    t0 = time.perf_counter()
    got = eng.psis_rows(ll)
    ms = 1e3 * (time.perf_counter() - t0)
    assert np.all(np.isfinite(got))
    assert got.tobytes() == eng.psis_rows(ll).tobytes()
    worst = _psis_check(got, ll, 'S=%d' % S)
    line = 'S_MAX = %d (M = 472, %d bytes of LDS): 7 rows in %.1f ms (with the copies), largest error / bound %.3e' % (
        S, pc.lds_bytes(472), ms, worst)
    print(line)
    RECORD['C'].append(line)
    RECORD['worst'] = max(RECORD['worst'], worst)
    # one more draw per row: refused in front of any copy or launch, and the device is as it was
    out = np.zeros((7, 3))
    more = pc.limit_rows(S + 1)
    assert eng.lib.epx_psis_rows(int(eng.device), 7, S + 1, _lib.dptr(more), _lib.dptr(out)) != 0
    msg = eng.lib.epx_last_error().decode()
    assert 'S = %d' % (S + 1) in msg and '473' in msg and 'LDS' in msg, msg
    assert not out.any()
    assert eng.psis_rows(pc.rows(50)).tobytes() == _device_rows(eng, 50).tobytes()


# ------------------------------------------------------------------ D. the two other consumers on duplicated draws
def _doubled(theta, seed):
    """(S, P) -> (S, P): the first ceil(S / 2) draws, each twice (S odd: the last of them once), permuted."""
    S = theta.shape[0]
    half = theta[:(S + 1) // 2]
    return np.ascontiguousarray(np.concatenate([half, half[:S // 2]])[np.random.RandomState(seed).permutation(S)])


@pytest.mark.parametrize('model', ['m4b_sg', 'm4a_sg'])
@pytest.mark.parametrize('S', [50, 226])
def test_loo_on_draws_that_occur_twice(model, S):
    D = 3
    X, y, k_lim = _rows_problem(model, D, 300 + D)
    e = HipEngine(model, X, y, k_lim)
    try:
        k = 2                                                           # 17 rows: a full tile and one past it
        theta = _doubled(0.5 * np.random.RandomState(S + is_gauss(model)).randn(S, e.P) + 0.3, S)
        assert len(np.unique(theta, axis=0)) == S // 2
        got = e.loo(k0=k, count=1, theta=theta[None])
        assert got.tobytes() == e.loo(k0=k, count=1, theta=theta[None]).tobytes()
        sl = slice(k_lim[k], k_lim[k + 1])
        worst = []
        _assert_loo_site(model, D, 1, theta, X[sl], None, y[sl], got, e, '%s S=%d twice' % (model, S), worst=worst)
        # twins carry the same log-likelihoods: the smoothed weights of a pair may swap, no sum over them changes
        flipped = e.loo(k0=k, count=1, theta=np.ascontiguousarray(theta[::-1])[None])
        np.testing.assert_allclose(flipped, got, rtol=1e-9, atol=1e-10)
        RECORD['D'].append('epx_loo %s S=%d, every draw twice: largest error / bound %.3e' % (model, S, max(worst)))
    finally:
        e.close()


def _twenty_fold(theta, seed):
    """(400, P) -> (400, P): the first 20 draws, each 20 times, permuted.  M = 60 and the bisection can count 20, 40, 60,
    80, ... draws, never 61 .. 76: the all-pairs route, and a tail of three whole levels above a fourth, which is smoothed
    (pairs, by contrast, always offer an even count inside the window: the listed route)."""
    assert theta.shape[0] == 400 and pc.tail_length(400) == 60 and pc.cand_cap(60) == 76
    return np.ascontiguousarray(np.tile(theta[:20], (20, 1))[np.random.RandomState(seed).permutation(400)])


@pytest.mark.parametrize('model', ['m4b_sg', 'm4a_sg'])
def test_loo_on_the_all_pairs_route(model):
    D, S, k = 3, 400, 2
    X, y, k_lim = _rows_problem(model, D, 300 + D)
    e = HipEngine(model, X, y, k_lim)
    try:
        theta = _twenty_fold(0.5 * np.random.RandomState(S + is_gauss(model)).randn(S, e.P) + 0.3, S)
        sl = slice(k_lim[k], k_lim[k + 1])
        mid, gauss = MODEL_IDS[model] % 5, is_gauss(model)
        ll = loo.loglik_host(mid, D, 1, gauss, theta, X[sl], np.zeros(17, dtype=np.int64), np.asarray(y[sl], dtype=np.float64))
        assert all(pc.route(r) == 'all-pairs' for r in ll)
        assert np.all(np.isfinite(loo.psis_host(ll)[:, 1]))               # and every row is smoothed
        got = e.loo(k0=k, count=1, theta=theta[None])
        assert got.tobytes() == e.loo(k0=k, count=1, theta=theta[None]).tobytes()
        worst = []
        _assert_loo_site(model, D, 1, theta, X[sl], None, y[sl], got, e, '%s S=%d twenty-fold' % (model, S), worst=worst)
        RECORD['D'].append('epx_loo %s S=%d, 20 draws 20 times each (all-pairs): largest error / bound %.3e' % (model, S, max(worst)))
    finally:
        e.close()


def test_reweight_on_the_all_pairs_route():
    """k_reweight's own use of the all-pairs branch: its tail_s entries and u slot (the log ratios of two cavities are
    tied exactly where the draws are)."""
    model, D, d, S = 'm1b_sg', 3, 4, 400
    case = Case(model, D, d, S, 0.1)
    try:
        theta = np.stack([_twenty_fold(case.theta[k], 7 + k) for k in range(2)])
        for prec_estim in ('sample', 'olse'):
            got = case.call(prec_estim, theta=theta)
            what = '%s d=%d S=%d twenty-fold %s' % (model, d, S, prec_estim)
            ratios, host = check_against_host(case, got, prec_estim, what, theta=theta)
            assert all(np.isfinite(h['khat']) for h in host)            # smoothed: every tail slot and tail_s entry is used
            assert same_bytes(got, case.call(prec_estim, theta=theta))
            RECORD['D'].append('epx_reweight_batch %s: %s' % (what, ' '.join('%s %.2e' % kv for kv in sorted(ratios.items()))))
    finally:
        case.close()


@pytest.mark.parametrize('model,D,d,S', [('m1b_sg', 3, 4, 64), ('m4b_sg', 8, 18, 203)])
def test_reweight_on_draws_that_occur_twice(model, D, d, S):
    case = Case(model, D, d, S, 0.1)
    try:
        theta = np.stack([_doubled(case.theta[k], 7 + k) for k in range(2)])
        assert all(len(np.unique(theta[k], axis=0)) == (S + 1) // 2 for k in range(2))
        for prec_estim in ('sample', 'olse'):
            got = case.call(prec_estim, theta=theta)
            what = '%s d=%d S=%d twice %s' % (model, d, S, prec_estim)
            ratios, host = check_against_host(case, got, prec_estim, what, theta=theta)
            assert all(np.isfinite(h['khat']) for h in host)            # smoothed: every tail slot and tail_s entry is used
            assert same_bytes(got, case.call(prec_estim, theta=theta))  # twice: the same bytes
            RECORD['D'].append('epx_reweight_batch %s: %s' % (what, ' '.join('%s %.2e' % kv for kv in sorted(ratios.items()))))
    finally:
        case.close()
