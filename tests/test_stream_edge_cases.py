"""(no device) The case table of the streaming sampler's edge tests, stream_edge_cases.py, against its own formulas, the
oracle and the library's LDS planning.

 * Every case has the geometry it claims: DPB, NV, (d, P), tiles per site, folds, ragged tiles -- so the device test
   runs the instantiations and the ring positions it says it runs, and not whatever a shape happens to select.
 * The C oracle, which the device is compared with, agrees at these shapes with the independent NumPy statement of the
   densities (1e-11, test_nuts_oracle.py's bound, for every single-group case of at most 100 rows; the value at 1e-10
   for the multi-group ones, whose NumPy statement has no gradient) and is finite at every gradient case, the
   saturated ones included.
 * Rounding robustness: wherever transitions or whole runs are compared, the strict and the fast oracle build take the
   same decisions to the end and their draws agree within 1e-9.  That is a condition on the table (a case that fails it
   gets another seed), so that a device kernel that parts from the oracle there has no rounding to plead.
 * The LDS bytes of every case and the first tile count the planner refuses (part D) are the library's own
   (tests/stream_plan_probe.hip calls nuts_stream_lds_bytes)."""

import subprocess

import numpy as np
import pytest

import stream_edge_cases as sc
from oracle import ep_oracle as eo
from oracle import nuts_oracle as no
from test_tree_endings_cases import _build_probe

CASES = sc.cases()
COMPARED = [c for c in CASES if c.compared]


def test_formulas_at_their_edges():
    assert [sc.dpb_of(D) for D in (1, 63, 64, 65, 127, 128)] == [64, 64, 64, 128, 128, 128]
    assert [sc.nv_of(P) for P in (1, 64, 65, 192, 193, 384, 385, 448)] == [1, 1, 2, 3, 4, 6, 7, 7]
    assert [sc.tiles_of(g) for g in ([1], [16], [17], [5, 1, 9], [4080], [4081])] == [1, 1, 2, 3, 255, 256]
    assert [sc.folds_of(t) for t in (1, 255, 256, 511, 512, 1025)] == [0, 0, 1, 1, 2, 4]
    assert sc.ragged_of([16, 17, 3]) == [(2, 1), (3, 3)]
    assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_case_has_the_geometry_it_claims(case):
    ng = max(len(s) for s in case.sites)
    assert no.dims(case.model, case.D, ng) == (case.d, case.P)
    if case.layout[1] == 4:
        assert case.dpb == (16 if case.D <= 16 else 32) and case.D <= 32          # (csrc/epx_api.hip plan_sampler: dpl)
    else:
        assert case.dpb == sc.dpb_of(case.D)
    assert case.nv == sc.nv_of(case.P) and case.nv <= 7
    assert case.multi == (ng > 1)
    for k, groups in enumerate(case.sites):
        assert case.tiles[k] == sc.tiles_of(groups)
        assert case.folds[k] == sc.folds_of(case.tiles[k])
        assert case.ragged[k] == sc.ragged_of(groups)
    p = sc.problem(case)
    assert p['P'] == case.P and p['d'] == case.d and p['X'].shape == (sum(sum(s) for s in case.sites), case.D)
    if case.part == 'B':
        for groups in case.sites:
            assert 40 <= sum(groups) <= 100 and sum(groups) % 16 != 0
    if case.compared:
        assert case.tight == sc.TIGHT


def test_table_holds_what_it_is_for():
    by = lambda part: sc.cases(part)
    # A: tile counts below, at and above the ring's look-ahead and length, for both families
    for model in ('m1b_sg', 'm4a_sg'):
        got = sorted((c.sites[0][0], c.tiles[0]) for c in by('A-tiles') if c.model == model)
        assert got == [(1, 1), (15, 1), (16, 1), (17, 2), (32, 2), (33, 3), (96, 6), (97, 7)]
    assert {t for t, _ in sc.TILE_COUNTS.values() if t < sc.RING_AHEAD} == {1, 2} and sc.NSL in {t for t, _ in sc.TILE_COUNTS.values()}
    # A: 255 tiles (no fold), 256 (the fold on the last, one-row tile), 257, and the counts beyond 1023 factors of 2
    assert sorted((c.model, c.D, c.sites[0][0], c.tiles[0], c.folds[0]) for c in by('A-folds')) == [
        ('m1b_sg', 33, 4080, 255, 0), ('m1b_sg', 33, 4081, 256, 1), ('m1b_sg', 33, 4097, 257, 1),
        ('m4b_sg', 8, 8200, 513, 2), ('m4b_sg', 8, 16400, 1025, 4)]
    assert [c.ragged[0] for c in by('A-folds') if c.tiles[0] == 256] == [[(255, 1)]]
    assert max(c.tiles[0] for c in by('A-folds')) > 1023
    # A: both sides of the DPB switch, one padding column, nearly only padding columns
    for model in ('m1b_sg', 'm4b_sg'):
        assert sorted((c.D, c.dpb) for c in by('A-cols') if c.model == model) == [(1, 64), (2, 64), (63, 64), (64, 64), (65, 128), (127, 128)]
    assert sorted(c.D for c in by('A-neighbour')) == [1, 33, 65]
    # B: one case per instantiation that no other test compares with a reference
    want = {(64, 3): 192, (64, 4): 195, (64, 5): 287, (64, 6): 357, (64, 7): 427, (128, 3): 129, (128, 4): 219, (128, 5): 258,
            (128, 6): 384}
    got = {}
    for c in by('B'):
        got.setdefault((c.dpb, c.nv), []).append(c.P)
        assert set(c.checks) == set(sc.SAMPLER)
    assert {k: min(v) for k, v in got.items()} == want and got[(128, 5)] == [258, 259]
    assert sorted(c.chains for c in by('B')) == [3, 4, 4, 4, 4, 4, 4, 4, 4, 6]
    # C: one to three tiles as a sampler, on the streaming default (D = 40) and beside the resident kernel (D = 8)
    assert sorted((c.D, c.sites[0][0], c.tiles[0]) for c in by('C')) == [(8, 1, 1), (8, 16, 1), (8, 17, 2), (8, 33, 3),
                                                                         (40, 1, 1), (40, 16, 1), (40, 17, 2), (40, 33, 3)]
    assert all(('resident' in c.checks) == (c.D == 8) for c in by('C'))
    (e,) = by('E')
    assert (e.model, e.D, e.P, e.nv, e.layout) == ('m4b', 32, 198, 4, (4, 4)) and [len(s) for s in e.sites] == [4, 4]


def _lane_log_product(factors, fold=True, keep_wlog=True):
    """The bookkeeping of ONE lane of the logistic wave (csrc/epx_stream_tile.h stream_pass_impl), restated: phase p
    multiplies the factor of tile p - 1 into the running product; with (p & 255) == 0 the product is folded into a sum
    of logarithms.  Returns log of the product of all factors as the kernel forms it."""
    wprod, wlog = 1.0, 0.0
    with np.errstate(over='ignore'):
        for p in range(1, len(factors) + 1):
            wprod = np.float64(wprod) * factors[p - 1]
            if fold and (p & (sc.FOLD_EVERY - 1)) == 0:
                wlog += np.log(wprod)
                wprod = 1.0
        return (wlog if keep_wlog else 0.0) + np.log(wprod)


def test_fold_cases_sit_where_the_fold_matters():
    """Why part A's fold cases have the tile counts they have, on a restatement of the lane's bookkeeping: at theta = 0
    every factor is exactly 2; the first fold comes with the 256th tile; a lane holds 1023 factors of 2 and no more, so
    the 1025-tile case is -inf without the fold; and a result that lost the folded sum is wrong from 256 tiles on and
    right at 255 -- the pair (4080, 4081 rows) brackets it."""
    for case in sc.cases('A-folds'):
        t = case.tiles[0]
        two = np.full(t, 2.0)
        want = t * np.log(2.0)
        assert abs(_lane_log_product(two) - want) <= 1e-13 * want, case.id
        lost = _lane_log_product(two, keep_wlog=False)
        assert (abs(lost - want) <= 1e-13 * want) == (case.folds[0] == 0), (case.id, lost, want)
        assert want - lost >= case.folds[0] * sc.FOLD_EVERY * np.log(2.0) * (1 - 1e-13)
        assert np.isfinite(_lane_log_product(two, fold=False)) == (t <= 1023), case.id
    assert np.isfinite(_lane_log_product(np.full(1023, 2.0), fold=False)) and np.isinf(_lane_log_product(np.full(1024, 2.0), fold=False))


GRAD_SMALL = [c for c in CASES if 'grad' in c.checks and max(sum(s) for s in c.sites) <= 100]


@pytest.mark.parametrize('case', GRAD_SMALL, ids=repr)
def test_oracle_gradient_agrees_with_the_numpy_statement(case):
    p = sc.problem(case)
    for k in range(case.K):
        lo, hi, gl = sc.site_rows(p, k)
        for th in sc.thetas(case, p, k):
            lp, g = sc.oracle_gradient(case, p, k, th)
            if case.multi:
                j_ind = np.repeat(np.arange(len(gl) - 1), np.diff(gl))
                lp2 = eo.site_logdensity_groups(case.model, th, p['X'][lo:hi], p['y'][lo:hi], j_ind, p['mus'][k], p['Oms'][k])
                assert abs(lp - lp2) < 1e-10 * max(1.0, abs(lp2)), (case.id, k, lp, lp2)
            else:
                lp2, g2 = eo.site_logdensity(case.model, th, p['X'][lo:hi], p['y'][lo:hi], p['mus'][k], p['Oms'][k])
                assert abs(lp - lp2) < 1e-11 * max(1, abs(lp2)), (case.id, k, lp, lp2)
                np.testing.assert_allclose(g, g2, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize('case', [c for c in CASES if 'grad' in c.checks], ids=repr)
def test_oracle_is_finite_at_every_gradient_case(case):
    scales = (1.0, sc.FOLD_ROW_SCALE) if case.part == 'A-folds' else (1.0,)
    for scale in scales:
        p = sc.problem(case, scale)
        for k in range(case.K):
            for th in sc.thetas(case, p, k):
                lp, g = sc.oracle_gradient(case, p, k, th)
                assert np.isfinite(lp) and np.all(np.isfinite(g)), (case.id, scale, k, lp)
                if case.part == 'A-folds' and not th.any():
                    # every row's factor is exactly 2 at theta = 0: the known answer of the likelihood term
                    n = case.sites[k][0]
                    v = -p['mus'][k]
                    want = -n * np.log(2.0) - 0.5 * v.dot(p['Oms'][k].dot(v))
                    assert abs(lp - want) <= 1e-12 * abs(want), (case.id, lp, want)


@pytest.mark.parametrize('case', COMPARED, ids=repr)
def test_strict_and_fast_builds_take_the_same_decisions(case):
    p = sc.problem(case)
    worst = 0.0
    if 'trans' in case.checks:
        (dr, st), (dr_f, st_f) = sc.oracle_transitions(case, p), sc.oracle_transitions(case, p, fast=True)
        assert np.all(st[:, :, 7] == 0) and st[:, :, 2].min() >= sc.NT
        for idx in (2, 3, 4):
            assert np.array_equal(st[:, :, idx], st_f[:, :, idx]), (case.id, 'transitions', idx, st[:, :, idx], st_f[:, :, idx])
        worst = max(worst, (np.abs(dr_f - dr).max(axis=(2, 3)) / np.maximum(1.0, np.abs(dr).max(axis=(2, 3)))).max())
    if 'run' in case.checks:
        (dr, st), (dr_f, st_f) = sc.oracle_run(case, p), sc.oracle_run(case, p, fast=True)
        assert np.all(st[:, :, 7] == 0)
        for idx in (2, 3, 4):
            assert np.array_equal(st[:, :, idx], st_f[:, :, idx]), (case.id, 'run', idx, st[:, :, idx], st_f[:, :, idx])
        worst = max(worst, (np.abs(dr_f - dr).max(axis=(2, 3)) / np.maximum(1.0, np.abs(dr).max(axis=(2, 3)))).max())
    print('%s: strict against fast build, largest draw difference %.3e (bound 1e-9)' % (case.id, worst))
    assert worst < 1e-9, (case.id, worst)


def test_lds_plan_of_every_case_is_the_librarys(tmp_path):
    """nuts_stream_lds_bytes at every case's shape: all fit (none is served by another form or refused), the tile table
    grows by 8 bytes per tile, and the first tile count the planner refuses at part D's shape is the table's."""
    exe = _build_probe(tmp_path, 'stream_plan_probe')
    cap = int(subprocess.check_output([exe, 'cap']))
    assert cap == 160 * 1024
    args = []
    for c in CASES:
        res = c.layout[1] == 4
        args += [c.nv, c.dpb, c.d, max(len(s) for s in c.sites), max(c.tiles), max(sum(s) for s in c.sites) if res else 0,
                 int(no.is_gauss(c.model))]
    out = [int(x) for x in subprocess.check_output([exe, 'bytes'] + [str(a) for a in args]).decode().split()]
    assert len(out) == len(CASES)
    for c, b in zip(CASES, out):
        print('%-40s LDS bytes %6d' % (c.id, b))
        assert b + (0 if c.layout[1] == 4 else sc.LDS_PIECE_BYTES) <= cap, (c.id, b)
    L = sc.LIMIT
    assert no.dims(L['model'], L['D']) == (L['d'], L['P']) and sc.dpb_of(L['D']) == L['dpb'] and sc.nv_of(L['P']) == L['nv']
    first, below, at = (int(x) for x in subprocess.check_output(
        [exe, 'first', str(L['nv']), str(L['dpb']), str(L['d']), '1', '0', str(sc.LDS_PIECE_BYTES)]).decode().split())
    assert first == L['first_refused_tiles']
    assert below + sc.LDS_PIECE_BYTES <= cap < at + sc.LDS_PIECE_BYTES
    # 8 bytes per tile, in 16-byte lines
    grow = [int(x) for x in subprocess.check_output(
        [exe, 'bytes'] + [str(a) for nt in (100, 102, 1100) for a in (L['nv'], L['dpb'], L['d'], 1, nt, 0, 0)]).decode().split()]
    assert grow[1] - grow[0] == 16 and grow[2] - grow[0] == 8000
    # the sites of part D (limit_problem): one tile below the limit and at it
    assert sc.tiles_of([sc.TR * first - 3]) == first and sc.tiles_of([sc.TR * (first - 1) - 3]) == first - 1
