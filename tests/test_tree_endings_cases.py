"""(no device) The case table of the tree-ending tests, tree_ending_cases.py, against the C oracle.

 * Every case has the endings it claims, from the strict oracle build: the device test then compares kernels with the
   oracle at endings that are known to be there, not at whatever a run happens to take.
 * Known answers of Stan 2.17's base_nuts::transition, asserted on the oracle (whose parity with Stan nothing else pins
   at these endings): a transition whose first leaf diverges or has a non-finite energy returns the start state bit for
   bit with accept statistic 0 (exp of an energy error below -1000, or of -inf, is 0 and the tree holds no other
   leaf); a transition at the cap has evaluated 2^10 - 1 leaves at depth 10; every leaf costs one gradient; and a run
   of nt transitions is its transitions one after the other -- its statistics are their sums and means.
 * Rounding robustness: the strict and the fast oracle build take the same decisions in every case.  That is a
   condition on the table (a case at which two CPU builds part is replaced), so that a device kernel that parts from
   the oracle at one of these cases has no rounding to plead."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import tree_ending_cases as tc
from oracle import nuts_oracle as no

CASES = tc.cases()
HERE = os.path.dirname(os.path.abspath(__file__))
_runs = {}


def _oracle(case, fast=False):
    key = (case.id, fast)
    if key not in _runs:
        p = tc.problem(case)
        runs = tc.oracle_runs(case, p, fast=fast)
        _runs[key] = (p, runs, tc.per_transition(runs))
    return _runs[key]


def _build_probe(tmp_path, name):
    """tests/<name>.hip compiled and linked with the tree's libepx.so; returns the program's path."""
    from epstan_amd import _lib
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'      # (the compiler that built the library)
    assert os.path.exists(_lib.LIB_PATH), 'libepx.so is not built'
    exe = str(tmp_path / name)
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O1', '-std=c++17', os.path.join(HERE, name + '.hip'), '-o', exe,
                           '-L' + libdir, '-l:' + os.path.basename(_lib.LIB_PATH), '-Wl,-rpath,' + libdir])
    return exe


def test_stack_plan_is_the_librarys(tmp_path):
    """tree_ending_cases.STACK_PLAN against the library's own LDS planning functions, called by a small program linked
    with libepx.so (tests/stack_plan_probe.hip): at (16, 48) the whole tree stack is in LDS, at (32, 500) it spills --
    layouts 1 and 5 keep all of it in global memory, layout 7 its levels 3 and up, from max_depth 3 on."""
    exe = _build_probe(tmp_path, 'stack_plan_probe')
    for (D, n), by_depth in tc.STACK_PLAN.items():
        d, P = no.dims('m4b_sg', D)
        for md, want in by_depth.items():
            out = subprocess.check_output([exe, str(P), str(d), str(D), str(n), str(md)]).decode().split('\n')
            got = {int(w[0]): (int(w[1]), int(w[2])) for w in (line.split() for line in out if line.strip())}
            assert got == want, ((D, n), md, got, want)
            assert all(int(line.split()[3]) <= 160 * 1024 for line in out if line.strip())        # (every form fits: none is replaced)
    # what the device test's cases rely on: every reduced depth and the cap chains' depth 10 are in the table
    for (D, n), layouts, depths in tc.DEPTH_RUN['shapes']:
        if (D, n) in tc.STACK_PLAN:
            assert set(depths) | {10} <= set(tc.STACK_PLAN[(D, n)])
    spill = tc.STACK_PLAN[(32, 500)]
    assert spill[2][7] == (1, 0) and spill[3][7] == (0, 3) and spill[4][7] == (0, 3)      # the depths 2 | 3 | 4 straddle both boundaries


def test_lds_plan_is_unchanged(tmp_path):
    """Every field the LDS planning functions write (nuts_lds_layout, nuts_duo_lds_layout) and nuts_stream_lds_bytes, over
    the sweep of tests/lds_plan_probe.hip, against tests/golden/lds_plan.txt -- the same program's output from the library
    as it was when the host wrote the kernels' record sizes out a second time (before csrc/nuts_geometry.h).  Line for
    line; the ALL line stands for the 15 120 plans of the whole cross product."""
    exe = _build_probe(tmp_path, 'lds_plan_probe')
    got = subprocess.check_output([exe]).decode().splitlines()
    with open(os.path.join(HERE, 'golden', 'lds_plan.txt')) as f:
        want = f.read().splitlines()
    assert len(want) == 1717 and sum(line.startswith('ALL 15120 ') for line in want) == 1
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i + 1, g, w)


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_case_has_the_endings_it_claims(case):
    p, runs, per = _oracle(case)
    assert np.all(runs[tc.NT][1][:, :, 7] == 0)
    tc.check_claims(case, p, per)
    lock = any(served in tc.LOCK_STEP for _, served in case.shape.layouts)
    for k in range(p['K']):
        kinds = {kind for c in range(p['C']) for kind in case.claims[k][c]}
        if lock:
            # a chain that ends at once beside one that runs to the cap, in one workgroup
            assert {'cap', 'first_leaf'} <= kinds, (case.id, k, kinds)


@pytest.mark.parametrize('shape', tc.SHAPES, ids=lambda s: '%s-c%d' % (s.key, s.chains))
def test_every_table_holds_every_kind(shape):
    kinds, longest_mid = set(), 0
    for tight in shape.tables:
        case = tc.Case(shape, tight)
        p, runs, per = _oracle(case)
        for k in range(p['K']):
            for c in range(p['C']):
                kinds |= set(case.claims[k][c])
                if 'mid_tree' in case.claims[k][c]:
                    longest_mid = max(longest_mid, int(per['leapfrogs'][k, c, 0]))
    assert kinds == set(tc.KINDS), (shape.key, kinds)
    assert longest_mid > 8, (shape.key, longest_mid)             # a divergence at least three doublings into the tree


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_first_leaf_endings_return_the_start_state(case):
    p, runs, per = _oracle(case)
    n = 0
    for k in range(p['K']):
        for c in range(p['C']):
            if not {'first_leaf', 'nonfinite'} & set(case.claims[k][c]):
                continue
            n += 1
            for nt in range(1, tc.NT + 1):
                dr, st = runs[nt]
                assert np.array_equal(dr[k, c], np.repeat(p['q0'][k, c][None, :], nt, axis=0)), (case.id, k, c, nt)
                assert st[k, c, 5] == 0.0 and st[k, c, 6] == 0.0, (case.id, k, c, st[k, c])
                assert st[k, c, 2] == nt and st[k, c, 3] == nt + 1 and st[k, c, 4] == nt, (case.id, k, c, st[k, c])
    assert n >= 2


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_run_of_transitions_is_its_transitions_one_after_the_other(case):
    """The nt = 3 run against three one-transition runs, each from the draw in front of it at its own place of the
    random stream: the same draws bit for bit, leapfrogs and divergences the sums, accept statistic and depth the means,
    one gradient per leaf and one at the start.  (So the differences of the nt = 1, 2, 3 statistics, which is all the
    device hook lets a test see, are the transitions' own figures.)"""
    p, runs, per = _oracle(case)
    s = case.shape
    q = p['q0']
    singles = []
    for t in range(tc.NT):
        dr, st = no.nuts_transitions(s.model, p['X'], p['y'], p['k_lim'], p['mus'], p['Oms'], tc.SEEDS, q, p['eps'], p['inv_e'],
                                     nt=1, t_offset=tc.T_OFFSET + t, g_cnt=p['g_cnt'], g_lim=p['g_lim'])
        singles.append((dr, st))
        q = dr[:, :, 0, :]
    for nt in range(1, tc.NT + 1):
        dr, st = runs[nt]
        assert np.array_equal(dr, np.concatenate([x[0] for x in singles[:nt]], axis=2))
        assert np.array_equal(dr, runs[tc.NT][0][:, :, :nt])
        for idx in (2, 4):
            assert np.array_equal(st[:, :, idx], sum(x[1][:, :, idx] for x in singles[:nt]))
        assert np.array_equal(st[:, :, 3], st[:, :, 2] + 1)                    # a gradient per leaf, one at the start
        for idx in (5, 6):
            np.testing.assert_allclose(st[:, :, idx], sum(x[1][:, :, idx] for x in singles[:nt]) / nt, rtol=1e-14, atol=0)
    for t in range(tc.NT):
        st = singles[t][1]
        assert np.array_equal(per['leapfrogs'][:, :, t], st[:, :, 2]) and np.array_equal(per['divergent'][:, :, t], st[:, :, 4])
        assert np.array_equal(per['depth'][:, :, t], st[:, :, 6])
        np.testing.assert_allclose(per['accept'][:, :, t], st[:, :, 5], rtol=0, atol=1e-14)
        # a tree of depth j without a discarded subtree has 2^j - 1 leaves; a discarded subtree adds at most 2^j more
        lf, dep = st[:, :, 2], st[:, :, 6]
        assert np.all(lf >= 2 ** dep - 1) and np.all(lf <= 2 ** (dep + 1) - 1), (case.id, t, lf, dep)
        assert np.all(lf[dep == 10] == tc.CAP_LEAPFROGS) and np.all(st[:, :, 4][dep == 10] == 0)
        assert np.all(lf[st[:, :, 4] == 1] > 2 ** dep[st[:, :, 4] == 1] - 1)   # a divergent leaf lies in a discarded subtree


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_strict_and_fast_builds_take_the_same_decisions(case):
    p, runs, per = _oracle(case)
    _, runs_f, per_f = _oracle(case, fast=True)
    for nt in range(1, tc.NT + 1):
        for idx in (2, 3, 4):                                                   # leapfrogs, gradients, divergences
            assert np.array_equal(runs[nt][1][:, :, idx], runs_f[nt][1][:, :, idx]), (case.id, nt, idx)
    assert np.array_equal(per['depth'], per_f['depth'])
    ref = runs[tc.NT][0]
    err = np.abs(runs_f[tc.NT][0] - ref).max(axis=(2, 3)) / np.maximum(1.0, np.abs(ref).max(axis=(2, 3)))
    assert np.all(err < 1e-6), (case.id, err)                                  # (the device test's bound; observed far below)


@pytest.mark.parametrize('D,n,md', [shape + (md,) for shape, _, depths in tc.DEPTH_RUN['shapes'] for md in depths])
def test_reduced_depth_runs_sit_at_the_cap(D, n, md):
    """The short runs the device test compares at a reduced max_treedepth: in the oracle's own trace at least a third of
    the transitions end at the cap (so does the part the device test gets to compare, which it checks itself), some end
    below it, and both oracle builds build the same trees."""
    r = tc.DEPTH_RUN
    X, y, k_lim, Oms, mus, P, seeds = tc.depth_run_problem(D, n)
    kw = dict(chains=r['chains'], iter=r['iter'], max_depth=md, trace_sites=r['K'])
    _, _, st, tr = no.nuts_sites(r['model'], X, y, k_lim, mus, Oms, seeds, **kw)
    with no.timing_build():
        _, _, st_f, tr_f = no.nuts_sites(r['model'], X, y, k_lim, mus, Oms, seeds, **kw)
    assert np.all(st[:, :, 7] == 0)
    cap = tc.at_cap(tr, md)
    assert 3 * cap.sum() >= cap.size, (md, cap.mean())
    assert tr[..., 3].max() == md and tr[..., 1].max() == 2 ** md - 1        # (a discarded subtree of depth j < md ends at most there)
    assert (tr[..., 4] == 1).any() and (md == 1 or ((tr[..., 4] == 0) & (tr[..., 3] < md)).any())
    for idx in (1, 3, 4):
        assert np.array_equal(tr[..., idx], tr_f[..., idx]), (md, idx)
