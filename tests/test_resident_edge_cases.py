"""(no device) The case table of the resident samplers' edge tests, resident_edge_cases.py, against the oracle's
dimensions and the library's own planning.

 * Every case has the geometry, the served layout and the kernel it claims: (d, P) against the oracle, DP and NV against
   their formulas, and the claim (family, homes of the cavity precision, the tree stack and the bookkeeping records, npad,
   tail columns, tiles per wave) against resident_edge_cases.plan -- plan_sampler's order of attempts restated over
   nuts_lds_layout / nuts_duo_lds_layout as tests/resident_plan_probe.hip calls them.  So the device test runs the
   instantiations it says it runs, and not whatever a shape happens to select.
 * Part H's row counts are the library's: a sweep over every site size finds the same boundaries, each pair straddles
   one, and the two sides differ.
 * Part I together with the committed coverage list (COVERED, recomputed here from the shapes of the earlier tests) is
   exactly the set of reachable instantiations; every family has a transition case; DESIGN.md carries the list.
 * Rounding robustness: at every transition case the strict and the fast oracle build take the same decisions and their
   draws agree within 1e-9 (a case that fails gets another seed), and where the tree stack has left the LDS some chain
   builds a tree deeper than the levels that stayed, so both homes are written and read.
 * The C oracle agrees with the independent NumPy statement of the densities at the gradient cases of at most 100 rows
   (test_nuts_oracle.py's 1e-11; the value at 1e-10 for several groups, whose NumPy statement has no gradient and covers
   the logistic programs only)."""

import os
import subprocess

import numpy as np
import pytest

import resident_edge_cases as rc
from oracle import ep_oracle as eo
from oracle import nuts_oracle as no
from test_tree_endings_cases import _build_probe

CASES = rc.cases()
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def lay(tmp_path_factory):
    exe = _build_probe(tmp_path_factory.mktemp('probe'), 'resident_plan_probe')
    assert int(subprocess.check_output([exe, 'cap'])) == rc.LDS_CAP
    return rc.Probe(exe)


def test_formulas_at_their_edges():
    assert [rc.pad_dp(D) for D in (1, 4, 5, 8, 9, 16, 17, 32, 33)] == [4, 4, 8, 8, 16, 16, 32, 32, -1]
    assert len({c.id for c in CASES}) == len(CASES)
    assert {c.chains for c in CASES if 'trans' in c.checks} == {4} and {c.chains for c in CASES if 'trans' not in c.checks} == {1}
    assert all(c.tight == rc.TIGHT for c in CASES if c.compared)


@pytest.mark.parametrize('part', sorted({c.part for c in CASES}))
def test_cases_have_the_geometry_and_the_kernel_they_claim(lay, part):
    for c in rc.cases(part):
        assert no.dims(c.model, c.D, max(c.ngmax, 1)) == (c.d, c.P), c.id
        assert c.dp == rc.pad_dp(c.D) and c.nv == (c.P + 63) // 64 and c.nv <= 2, c.id
        r = c.plan(lay)
        assert (r['served'], rc.claim_of(r)) == (c.served, c.claim), (c.id, r)
        assert 0 < r['lds_bytes'] <= rc.LDS_CAP or c.served == 3, (c.id, r)
        if c.claim[0].startswith('duo') and c.claim[0] != 'duo44':
            dm, ou = min(c.d, 64), (4 if c.nv > 1 else 8)                   # (csrc/nuts_geometry.h duo_ou; nuts_duo_lds_layout's npad)
            assert c.claim[5] == ((dm + 1) // 2 + ou - 1) // ou * ou and c.claim[6] == max(c.d - 64, 0), c.id
        if c.claim[0] == 'duo44':
            t = ((c.n_max + 15) // 16 + 3) // 4                             # (csrc/nuts_duo.hip team_tiles_per_wave)
            assert c.claim[7] == (t + 1) & ~1, c.id
        if 'grad' in c.checks or 'neighbour' in c.checks:
            p = rc.problem(c) if c.n_max <= 100 else None
            assert p is None or (p['P'] == c.P and p['d'] == c.d and list(np.diff(p['k_lim'])) == c.rows), c.id


def test_part_h_sits_on_the_librarys_boundaries(lay):
    for table, chains in ((rc.H_GRAD, 1), (rc.H_TRANS, 4)):
        for (model, req), rows in table.items():
            plans, changes = rc.sweep(lay, model, 32, req, chains)
            if chains == 4:      # the transition pairs: where the stack leaves the LDS and a resident kernel still serves
                changes = [n for n in changes if plans[n]['st'] != plans[n - 1]['st'] and plans[n]['served'] != 3]
            ns = [n for n, _, _ in rows]
            print('%s layout %d, %d chain(s): the plan changes at %s rows' % (model, req, chains, changes))
            assert ns[1::2] == changes and ns[0::2] == [n - 1 for n in changes], (model, req, chains, changes, ns)
            for (n0, s0, c0), (n1, s1, c1) in zip(rows[0::2], rows[1::2]):
                assert (s0, c0) != (s1, c1), (model, req, n1)
                if chains == 4:
                    assert (c0[2], c1[2]) == (1, 0), (model, req, n1)
    # every resident layout, both logistic models and a Gaussian one; the pairs where a request stops being served
    assert {k for k in rc.H_GRAD} == {(m, l) for m in ('m4b_sg', 'm1b_sg') for l in (1, 2, 5, 6, 7)} | {('m4a_sg', l) for l in (0, 1, 2)}
    assert rc.H_GRAD[('m4a_sg', 0)][-1][1] == 3 and all(rows[-1][1] == 3 for rows in rc.H_GRAD.values())
    assert [s for _, s, _ in rc.H_GRAD[('m1b_sg', 7)]] == [7, 7, 7, 5, 5, 2, 2, 3]
    # the layout-1 site with the cavity precision read from L2, and layout 2 without room for the bookkeeping records
    assert rc.W1_NONE in [c for _, _, c in rc.H_GRAD[('m4b_sg', 1)]]
    assert {rc.W4_RES, rc.W4_GLB} <= {c for _, _, c in rc.H_GRAD[('m4b_sg', 2)]}


def test_every_reachable_instantiation_has_a_reference_test(lay):
    covered = rc.covered_by_existing(lay)
    assert covered == rc.COVERED
    reach = rc.reachable(lay)
    part_i = {rc.instantiation_of_claim(c) for c in rc.cases('I', 'grad')}
    for c in rc.cases('I'):
        assert rc.instantiation(c.plan(lay)) == rc.instantiation_of_claim(c), c.id
    for k in sorted(reach):
        print('%-40s %s' % (k, rc.COVERED.get(k) or 'part I'))
    assert not part_i & set(covered) and part_i | set(covered) == reach, (sorted(reach - part_i - set(covered)), sorted(part_i - reach))
    assert len(part_i) == len(rc.cases('I', 'grad'))
    # the group kernel with two registers per chain vector at DP = 4 and 8
    assert {('spec-grp', 2, 4, 0), ('spec-grp', 2, 8, 0)} <= part_i
    # one transition case per family
    fams = {rc.instantiation_of_claim(c)[0] for c in rc.cases('I', 'trans')}
    assert fams == {k[0] for k in reach}, fams
    with open(os.path.join(HERE, '..', 'DESIGN.md')) as f:
        design = f.read()
    for line in rc.design_lines():
        assert line in design, line


def test_table_holds_what_it_is_for():
    by = lambda part: rc.cases(part)
    for model in ('m4b_sg', 'm1b_sg'):
        assert sorted({c.D for c in by('C-dp') if c.model == model}) == [1, 2, 4, 5, 8, 9, 15, 16, 17, 31, 32]
        for D in (1, 2, 4, 5, 8):
            assert sorted(c.req for c in by('C-dp') if c.model == model and c.D == D) == [1, 2]
        for D in (9, 15, 16, 17, 31, 32):
            assert sorted(c.req for c in by('C-dp') if c.model == model and c.D == D) == [1, 2, 5, 6, 7]
    # every shape of the four models with P in 63 .. 66 or d in 62 .. 66 is in part C
    want = {(m, D) for m in ('m4b_sg', 'm3b_sg', 'm4a_sg', 'm3a_sg') for D in range(1, 33)
            if no.dims(m, D)[1] in (63, 64, 65, 66) or no.dims(m, D)[0] in (62, 63, 64, 65, 66)}
    assert want == {(c.model, c.D) for c in by('C-reg')} | {('m4b_sg', 31), ('m4b_sg', 32)}
    assert {c.P for c in by('C-reg')} >= {63, 64, 65, 66} and {c.d for c in by('C-reg') + by('C-dp')} >= {62, 63, 64, 65, 66}
    # the tail of the row-wave kernels: zero columns at NV = 2 (d = 64) and two (d = 66); d = 65 is no logistic shape
    assert {(c.d, c.claim[6]) for c in by('C-dp') if c.claim[0].startswith('duo') and c.nv == 2} == {(64, 0), (66, 2)}
    assert not [m for m in rc.SG_B for D in range(1, 33) if no.dims(m, D)[0] == 65]
    (c,) = by('C-d2')
    assert (c.d, c.req, c.claim) == (2, 2, rc.S_RES)
    assert sorted((c.req, c.n_max) for c in by('R-rows')) == [(1, 1), (1, 63), (1, 64), (1, 65), (2, 1), (2, 255), (2, 256), (2, 257),
                                                            (6, 1), (6, 255), (6, 256), (6, 257)]
    for c in by('R-ragged'):
        assert c.rows[0] == 1 and c.rows[1] == max(n for n, s, _ in rc.H_GRAD[('m4b_sg', c.req)] if s == c.req) and c.served == c.req
    assert sorted((c.D, c.req) for c in by('N')) == [(D, l) for D in (1, 5, 17) for l in (1, 2, 5, 7)]
    assert all('neighbour' in c.checks for c in by('N') + by('R-ragged'))


def test_factor_count_of_the_largest_dp4_site(lay):
    (c,) = rc.cases('R-factors')
    plans, _ = rc.sweep(lay, c.model, c.D, 1, 1)
    assert c.n_max == max(n for n in range(1, len(plans)) if plans[n]['served'] == 1) == rc.FACTORS['n']
    assert -(-c.n_max // 64) == rc.FACTORS['factors'] <= rc.MAX_FACTORS
    # at theta = 0 every row's factor is exactly 2: the known answer of the likelihood term
    p = rc.problem(c)
    lp, g = rc.oracle_gradient(c, p, 0, np.zeros(c.P))
    v = -p['mus'][0]
    want = -c.n_max * np.log(2.0) - 0.5 * v.dot(p['Oms'][0].dot(v))
    assert abs(lp - want) <= 1e-12 * abs(want), (lp, want)


GRAD_SMALL = [c for c in CASES if 'grad' in c.checks and c.n_max <= 100]


@pytest.mark.parametrize('part', sorted({c.part for c in GRAD_SMALL}))
def test_oracle_gradient_agrees_with_the_numpy_statement(part):
    for case in [c for c in GRAD_SMALL if c.part == part]:
        p = rc.problem(case)
        for k in range(case.K):
            lo, hi, gl = rc.site_rows(p, k)
            for th in rc.thetas(case, p, k):
                lp, g = rc.oracle_gradient(case, p, k, th)
                assert np.isfinite(lp) and np.all(np.isfinite(g)), (case.id, k)
                if case.multi and case.gauss:
                    continue                                             # (no NumPy statement of the Gaussian multi-group programs: finite only)
                if case.multi:
                    j_ind = np.repeat(np.arange(len(gl) - 1), np.diff(gl))
                    lp2 = eo.site_logdensity_groups(case.model, th, p['X'][lo:hi], p['y'][lo:hi], j_ind, p['mus'][k], p['Oms'][k])
                    assert abs(lp - lp2) < 1e-10 * max(1.0, abs(lp2)), (case.id, k, lp, lp2)
                else:
                    lp2, g2 = eo.site_logdensity(case.model, th, p['X'][lo:hi], p['y'][lo:hi], p['mus'][k], p['Oms'][k])
                    assert abs(lp - lp2) < 1e-11 * max(1, abs(lp2)), (case.id, k, lp, lp2)
                    np.testing.assert_allclose(g, g2, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize('case', rc.cases(check='trans'), ids=repr)
def test_strict_and_fast_builds_take_the_same_decisions(case):
    p = rc.problem(case)
    runs, runs_f = rc.oracle_transitions(case, p), rc.oracle_transitions(case, p, fast=True)
    worst = 0.0
    for nt in (1, 2, 3):
        (dr, st), (dr_f, st_f) = runs[nt], runs_f[nt]
        assert np.all(st[:, :, 7] == 0) and st[:, :, 3].min() >= nt
        for idx in (2, 3, 4, 6):
            assert np.array_equal(st[:, :, idx], st_f[:, :, idx]), (case.id, nt, idx, st[:, :, idx], st_f[:, :, idx])
        assert np.all(np.abs(st[:, :, 5] - st_f[:, :, 5]) <= 1e-9 + 1e-9 * np.abs(st[:, :, 5])), case.id
        worst = max(worst, (np.abs(dr_f - dr).max(axis=(2, 3)) / np.maximum(1.0, np.abs(dr).max(axis=(2, 3)))).max())
    dep = rc.depths(runs)
    print('%s: strict against fast build, largest draw difference %.3e (bound 1e-9); tree depths %s' % (case.id, worst, dep.reshape(-1, 3).tolist()))
    assert worst < 1e-9, (case.id, worst)
    assert dep.min() >= 1
    if case.part == 'H' and not case.claim[2]:
        # the stack has left the LDS: some chain builds a tree deeper than the levels that stayed there
        assert dep.max() > case.claim[3], (case.id, dep.max(), case.claim[3])
