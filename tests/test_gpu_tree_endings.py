"""How every sampler layout ENDS a tree: at the depth cap, at a divergent leaf (the first one, or one inside a later
subtree), at a leaf whose energy is not finite, and at a U-turn -- forced chain by chain inside one site through the
per-chain step sizes of epx_nuts_transitions (tree_ending_cases.py: the table, checked against the oracle without a
device by test_tree_endings_cases.py).

nuts_state_machine.inc is shared by the layouts; what surrounds it is not (a speculative bookkeeping wave in layout 2,
the two-entry mailbox of layout 6, the tree one leapfrog behind the integration in layout 7, lock-step partners that
run on beside an ended chain in layouts 3 / 4 / 7, and -- at the one shape of the table where the stack spills,
(32, 500): tree_ending_cases.STACK_PLAN -- a tree stack that is wholly in global memory for layouts 1 and 5 and has its
levels 3 and up there for layout 7; at the small shapes the stack is wholly in LDS for layouts 1 2 5 6 7 and wholly in
global memory for layouts 3 4, no boundary is crossed).  Per (case, layout): the oracle runs at the device's own cavities and must still show
the claimed endings; the device takes nt = 1, 2, 3 transitions with the requested layout (a request served by another
layout is an error).  The bounds are the ones the existing tests of the same hooks use:

  * leapfrogs, gradients, divergences per chain and the mean depth: equal;
  * every draw: 1e-6 relative to max(1, |ref|), the teacher-forced bound of test_gpu_parity, no chain excepted;
  * the draws of a first-leaf or non-finite ending: the start state bit for bit;
  * the mean accept statistic: 1e-9 + 1e-9 |ref| (test_gpu_round5's teacher-forced bound);
  * the same launch again: the same bits.

Then whole short runs at a reduced max_treedepth against the oracle's trace (test_gpu_round5's parting-transition
comparison), at least a third of the compared transitions at the cap: depths 1, 3, 4 at the small shapes (the cap
itself), and 2, 3, 4 at (32, 500), where layout 7's stack is whole in LDS, split with every level in LDS, and split
with level 3 in the global store (the boundary is asserted on the library by test_tree_endings_cases.py)."""

import numpy as np
import pytest

import tree_ending_cases as tc
from epstan_amd.engine import HipEngine
from oracle import nuts_oracle as no
from test_gpu_parity import _engine_with_cavity, _group_engine
from test_gpu_round5 import _parting

pytestmark = pytest.mark.gpu

_setups = {}


def _setup(case):
    """Engine at the case's cavities, and the oracle's nt = 1, 2, 3 runs at the cavities the device holds; shared by the
    layouts of a case."""
    if case.id not in _setups:
        p = tc.problem(case)
        s = case.shape
        if s.groups is None:
            eng, Om_dev, mu_dev = _engine_with_cavity(s.model, p['X'], p['y'], p['k_lim'], p['Oms'], p['mus'])
        else:
            eng, Om_dev, mu_dev = _group_engine(s.model, p['X'], p['y'], p['k_lim'], p['g_cnt'], p['g_lim'], p['Oms'], p['mus'])
        assert eng.P == p['P']
        runs = tc.oracle_runs(case, p, Om_dev, mu_dev)
        per = tc.per_transition(runs)
        tc.check_claims(case, p, per, Om_dev, mu_dev)
        _setups[case.id] = (p, eng, runs, per)
    return _setups[case.id]


PAIRS = [(case, req, served) for case in tc.cases() for req, served in case.shape.layouts]


@pytest.mark.parametrize('case,req,served', PAIRS, ids=['%r-layout%d' % (c, s) for c, r, s in PAIRS])
def test_layout_ends_trees_as_the_oracle_does(case, req, served):
    p, eng, runs, per = _setup(case)
    K, C = p['K'], p['C']
    dev = {}
    for nt in (1, 2, 3, 3):
        o, st = eng.nuts_transitions(tc.SEEDS, p['q0'], p['eps'], p['inv_e'], nt=nt, t_offset=tc.T_OFFSET, layout=req)
        assert eng.last_layout() == served, (case.id, req, eng.last_layout())
        if nt in dev:
            np.testing.assert_array_equal(o, dev[nt][0])                        # (the same launch again: the same bits)
            np.testing.assert_array_equal(st, dev[nt][1])
        dev[nt] = (o, st)
    per_d = tc.per_transition(dev, whole=False)
    print('%s layout %d: leapfrogs per transition, oracle %s device %s' % (case.id, served, per['leapfrogs'].reshape(K * C, -1).tolist(),
                                                                           per_d['leapfrogs'].reshape(K * C, -1).tolist()))
    worst_draw = worst_acc = 0.0
    for nt in (1, 2, 3):
        (o, st), (ref, st_o) = dev[nt], runs[nt]
        assert np.all(st[:, :, 7] == 0)
        for idx, name in ((2, 'leapfrogs'), (3, 'gradients'), (4, 'divergences'), (6, 'mean depth')):
            assert np.array_equal(st[:, :, idx], st_o[:, :, idx]), (case.id, served, nt, name, st[:, :, idx], st_o[:, :, idx])
        assert np.all(np.isfinite(o))
        err = np.abs(o - ref).max(axis=(2, 3)) / np.maximum(1.0, np.abs(ref).max(axis=(2, 3)))
        acc = np.abs(st[:, :, 5] - st_o[:, :, 5]) / (1e-9 + 1e-9 * np.abs(st_o[:, :, 5]))
        worst_draw, worst_acc = max(worst_draw, err.max()), max(worst_acc, acc.max())
        print('%s layout %d nt %d: largest draw difference %.3e (bound 1e-6), accept difference %.3e of its bound'
              % (case.id, served, nt, err.max(), acc.max()))
        assert np.all(err < 1e-6), (case.id, served, nt, err)
        assert np.all(acc <= 1.0), (case.id, served, nt, st[:, :, 5], st_o[:, :, 5])
        for k in range(K):
            for c in range(C):
                if {'first_leaf', 'nonfinite'} & set(case.claims[k][c]):
                    assert np.array_equal(o[k, c], np.repeat(p['q0'][k, c][None, :], nt, axis=0)), (case.id, served, nt, k, c)
                    assert st[k, c, 5] == 0.0
    print('MARGIN %s layout %d: draws %.3e accept %.3e' % (case.id, served, worst_draw, worst_acc))


# ---------------------------------------------------------------- max_treedepth below 10
_depth_refs = {}
_depth_engines = {}

DEPTH_CASES = [(D, n, layout, md) for (D, n), layouts, depths in tc.DEPTH_RUN['shapes'] for layout in layouts for md in depths]


@pytest.mark.parametrize('D,n,layout,md', DEPTH_CASES)
def test_short_runs_at_a_reduced_depth_cap_follow_the_oracle(D, n, layout, md):
    r = tc.DEPTH_RUN
    K, C, it, model = r['K'], r['chains'], r['iter'], r['model']
    if (D, n) not in _depth_engines:
        X, y, k_lim, Oms, mus, P, seeds = tc.depth_run_problem(D, n)
        eng, Om_dev, mu_dev = _engine_with_cavity(model, X, y, k_lim, Oms, mus)
        _depth_engines[(D, n)] = (eng, X, y, k_lim, Om_dev, mu_dev, P, seeds)
    eng, X, y, k_lim, Om_dev, mu_dev, P, seeds = _depth_engines[(D, n)]
    if (D, n, md) not in _depth_refs:
        _depth_refs[(D, n, md)] = no.nuts_sites(model, X, y, k_lim, mu_dev, Om_dev, seeds, chains=C, iter=it, max_depth=md,
                                                trace_sites=K)[3]
    tr_o = _depth_refs[(D, n, md)]
    opts = HipEngine.sampler_opts(chains=C, iter=it, warmup=None, init='random', max_depth=md, layout=layout)
    eng.set_trace(K)
    try:
        eng.sample_batch(seeds, opts)
        assert eng.last_layout() == layout
        tr_d = eng.get_trace(C, it)
    finally:
        eng.set_trace(0)
    t_star, before, err = _parting(tr_d, tr_o)
    n_cmp = n_cap = 0
    assert tr_o[..., 3].max() <= md and tr_d[..., 3].max() <= md
    for k in range(K):
        for c in range(C):
            ts = int(t_star[k, c])
            assert before[k, c] < 1e-6, (layout, md, k, c, ts, before[k, c])
            for t in range(ts):
                a, b = tr_d[k, c, t], tr_o[k, c, t]
                assert a[1] == b[1] and a[3] == b[3] and a[4] == b[4], (layout, md, k, c, t, a[:8], b[:8])
            n_cmp += ts
            n_cap += int(tc.at_cap(tr_o[k, c, :ts], md).sum())
    # the first transition -- the step-size search from eps = 1 included -- agrees to rounding
    assert err[:, :, 0].max() < 1e-9 and np.abs(tr_d[:, :, 0, 5] / tr_o[:, :, 0, 5] - 1.0).max() < 1e-9
    print('DEPTH D=%d n=%d layout %d max_depth %d: %d of %d transitions compared, %d at the cap, error in front of the partings %.3e'
          % (D, n, layout, md, n_cmp, K * C * it, n_cap, before.max()))
    # not vacuous (test_gpu_round5's requirement): most chains get through the step-size search and several transitions
    # together; and at least a third of what was compared sits at the cap
    assert np.median(t_star) >= 3 and n_cmp >= 3 * K * C, (t_star, n_cmp)
    assert 3 * n_cap >= n_cmp, (n_cap, n_cmp)
