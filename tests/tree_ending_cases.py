"""The case table of the tree-ending tests (plain helper, no tests): test_tree_endings_cases.py (no device) and
test_gpu_tree_endings.py (device) share it.

A NUTS transition ends with a U-turn, at the max_treedepth cap, at a divergent leaf (energy error above 1000) or at a
leaf whose energy is not finite (Stan 2.17 maps a NaN energy to +inf: the leaf is divergent).  The teacher-forced hook
(epx_nuts_transitions / epo_nuts_transitions) takes a step size per (site, chain), so one launch holds every ending side
by side: each case multiplies the step sizes of a 40-iteration ORACLE run (nothing here depends on the device) chain by
chain --
    x 1e-2 (1e-3)   the trajectory never turns round:   1 023 leapfrogs, depth 10           `cap`
    x 3 .. 10       the first leaf's energy error > 1000: 1 leapfrog, the start state kept  `first_leaf`
    x 1e6           the first leaf overflows: log density or gradient inf / NaN             `nonfinite` (and `first_leaf`)
    x 1 .. 10       a leaf inside a later subtree diverges: that subtree is discarded whole  `mid_tree`
    x 1 .. 3        an ordinary transition                                                   `uturn`
-- and names per chain what the FIRST of the nt = 3 transitions does (`cap`, `first_leaf` and `nonfinite` hold for all
three: a chain that keeps its start state meets the same wall again).  The claims are checked against the strict oracle
build by test_tree_endings_cases.py, and again by the device test on the oracle run at the device's own cavities."""

import numpy as np

from oracle import nuts_oracle as no
from test_gpu_parity import _group_problem, _site_problem

NT = 3
T_OFFSET = 4
SEEDS = np.array([21, 22], dtype=np.int64)
CAP_LEAPFROGS = 1023                # 2^10 - 1: max_treedepth = 10, the depth epx_nuts_transitions runs with
KINDS = ('cap', 'first_leaf', 'mid_tree', 'nonfinite', 'uturn')
LOCK_STEP = (3, 4, 7)               # layouts whose chains share a pass: an ended chain sits beside ones that run on

_C, _F, _M, _N, _U = ('cap',), ('first_leaf',), ('mid_tree',), ('first_leaf', 'nonfinite'), ('uturn',)


class Shape:
    """A site shape, the layouts that run it as (requested, served) pairs, and per cavity tightness the step-size
    multipliers [site][chain] with the ending each chain claims."""

    def __init__(self, key, model, D, layouts, n=None, groups=None, chains=4, tables=None):
        self.key, self.model, self.D, self.n, self.groups, self.chains = key, model, D, n, groups, chains
        self.layouts = tuple((L, L) if isinstance(L, int) else L for L in layouts)
        self.tables = tables


def _table(*sites):
    """[(multiplier, claim), ...] per site -> (multipliers, claims)."""
    return [[m for m, _ in s] for s in sites], [[c for _, c in s] for s in sites]


SHAPES = [
    # the smallest shape every resident kernel has: dp = 16, three row tiles
    Shape('m4b_sg-16-48', 'm4b_sg', 16, (1, 2, 4, 5, 6, 7), n=48,
          tables={1.0: _table([(1e-2, _C), (3, _F), (1, _M), (1e6, _N)], [(10, _F), (1e-2, _C), (1e6, _N), (3, _M)]),
                  1000.0: _table([(1e-2, _C), (3, _U), (1, _U), (1e6, _N)], [(10, _M), (1e-2, _C), (1e6, _N), (3, _U)])}),
    # streaming: three row tiles are the ring's look-ahead; P = 123, NV = 2
    Shape('m4b_sg-40-48', 'm4b_sg', 40, (3,), n=48,
          tables={1.0: _table([(1e-3, _C), (3, _F), (3, _M), (1e6, _N)], [(10, _F), (1e-3, _C), (1, _M), (1e6, _N)]),
                  1000.0: _table([(1e-3, _C), (3, _U), (10, _F), (1e6, _N)], [(10, _M), (1e-3, _C), (1e6, _N), (10, _F)])}),
    # the state wave's plain path (no per-coefficient scales)
    Shape('m1b_sg-16-48', 'm1b_sg', 16, (1, 7), n=48,
          tables={1.0: _table([(1e-3, _C), (10, _F), (1e6, _N), (1, _U)], [(1, _M), (1e6, _N), (1e-3, _C), (10, _F)]),
                  1000.0: _table([(1e6, _N), (10, _F), (1e-3, _C), (1, _U)], [(1e6, _N), (1e-3, _C), (1, _U), (10, _F)])}),
    # the Gaussian-likelihood family on its resident kernels
    Shape('m4a_sg-16-48', 'm4a_sg', 16, (1, 2), n=48,
          tables={1.0: _table([(1.5, _M), (3, _F), (1e6, _N), (1e-3, _C)], [(1, _U), (1e-3, _C), (1, _M), (1e6, _N)]),
                  1000.0: _table([(1, _U), (1e-3, _C), (10, _M), (1e6, _N)], [(10, _F), (1e-3, _C), (10, _M), (1, _U)])}),
    # the Gaussian-likelihood family streamed: the default of a shape its resident kernels do not take
    Shape('m4a_sg-40-48', 'm4a_sg', 40, ((0, 3),), n=48,
          tables={1.0: _table([(1e-3, _C), (1, _M), (10, _F), (1e6, _N)], [(10, _F), (1e-3, _C), (1, _M), (1, _U)]),
                  1000.0: _table([(10, _F), (1, _U), (1e-3, _C), (1e6, _N)], [(10, _F), (10, _M), (1e-3, _C), (1e6, _N)])}),
    # multi-group sites (three and two groups: the second site zero padded), the shape of
    # test_multigroup_site_updates_match_oracle; layout 2 in its group form
    Shape('m4b-4-groups', 'm4b', 4, (2, 3, 4), groups=[[20, 14, 9], [25, 25]],
          tables={1.0: _table([(2, _M), (3, _F), (1e-3, _C), (1e6, _N)], [(10, _F), (1e-3, _C), (1e6, _N), (2, _M)]),
                  1000.0: _table([(10, _F), (1, _U), (3, _M), (1e-3, _C)], [(10, _M), (10, _F), (1e6, _N), (1e-3, _C)])}),
    # a lock-step workgroup with one chain missing
    Shape('m4b_sg-16-48', 'm4b_sg', 16, (7, 3, 4), n=48, chains=3,
          tables={1.0: _table([(2, _M), (3, _F), (1e-2, _C)], [(10, _F), (1e-2, _C), (1e6, _N)]),
                  1000.0: _table([(1e-2, _C), (3, _U), (1e6, _N)], [(10, _M), (1e-2, _C), (10, _F)])}),
    # the headline site shape: the rows fill the LDS, so the tree stack SPILLS -- layout 7 keeps levels 0 .. 2 in LDS and
    # the levels above in its per-workgroup global store, layouts 5 and 1 keep all of it there (STACK_PLAN below); the
    # mid-tree divergence of the first cavity comes 201 leapfrogs into its transition, behind seven doublings
    Shape('m4b_sg-32-500', 'm4b_sg', 32, (7, 5, 1), n=500,
          tables={1.0: _table([(1e-2, _C), (3, _F), (3, _U), (1e6, _N)], [(5, _F), (1, _M), (1e-2, _C), (1e6, _N)]),
                  1000.0: _table([(1e-2, _C), (1, _U), (1e6, _N), (1, _U)], [(1e-2, _C), (1, _U), (1e6, _N), (10, _F)])}),
]

# Where the library's LDS planning (csrc/nuts.hip nuts_lds_layout, csrc/nuts_duo.hip nuts_duo_lds_layout, as
# csrc/epx_api.hip plan_sampler calls them) puts the tree stack of a 4-chain launch of the resident layouts 1, 5, 7:
# {(D, n): {max_depth: {layout: (whole stack in LDS, lowest levels in LDS when it is not)}}}.  At (16, 48) the whole
# stack is in LDS whatever the depth (so it is for layouts 2 and 6, one chain per workgroup); the lock-step layouts 3
# and 4 keep the whole stack in global memory at every shape.  At (32, 500) it spills.  test_tree_endings_cases.py
# checks this table against the library's own functions (tests/stack_plan_probe.hip), so the depths of the reduced-cap
# runs below sit at a boundary that is there.
STACK_PLAN = {
    (16, 48): {md: {1: (1, 0), 5: (1, 0), 7: (1, 0)} for md in (1, 3, 4, 10)},
    (32, 500): {2: {1: (0, 0), 5: (0, 0), 7: (1, 0)},          # layout 7: two levels still fit as a whole stack
                3: {1: (0, 0), 5: (0, 0), 7: (0, 3)},          # ... three do not: the split form, every level in LDS
                4: {1: (0, 0), 5: (0, 0), 7: (0, 3)},          # ... level 3 is the first in the global store
                10: {1: (0, 0), 5: (0, 0), 7: (0, 3)}},        # the cap chains: every level above 2 there
}


class Case:
    def __init__(self, shape, tight):
        self.shape, self.tight = shape, tight
        mult, claims = shape.tables[tight]
        self.mult = np.array(mult, dtype=np.float64)
        self.claims = claims
        assert self.mult.shape == (2, shape.chains)
        self.id = '%s-c%d-tight%g' % (shape.key, shape.chains, tight)

    def __repr__(self):
        return self.id


def cases():
    return [Case(s, t) for s in SHAPES for t in sorted(s.tables)]


_problems = {}


def problem(case):
    """The sites, their nominal cavities, and q0 / eps / inv_e from the oracle's own 40-iteration run: the last kept
    draw, the adapted step size times the case's multiplier, and the site's pooled variance + 1e-6."""
    if case.id in _problems:
        return _problems[case.id]
    s = case.shape
    K, C = 2, s.chains
    g_cnt = g_lim = None
    if s.groups is None:
        X, y, k_lim, Oms, mus, d, P = _site_problem(s.model, s.D, s.n, 400 + s.D + s.n, K=K, tight=case.tight)
    else:
        X, y, k_lim, g_cnt, g_lim, Oms, mus, d = _group_problem(s.model, s.D, s.groups, 70 + s.D, tight=case.tight)
        P = no.dims(s.model, s.D, int(g_cnt.max()))[1]
    draws, _, st = no.nuts_sites(s.model, X, y, k_lim, mus, Oms, SEEDS, chains=C, iter=40, g_cnt=g_cnt, g_lim=g_lim)
    assert np.all(st[:, :, 7] == 0)
    inv_e = np.repeat(draws.reshape(K, -1, P).var(axis=1)[:, None, :], C, axis=1) + 1e-6
    p = dict(X=X, y=y, k_lim=k_lim, g_cnt=g_cnt, g_lim=g_lim, Oms=Oms, mus=mus, P=P, K=K, C=C,
             q0=draws[:, :, -1, :].copy(), eps=st[:, :, 1] * case.mult, inv_e=inv_e)
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _problems[case.id] = p
    return p


def oracle_runs(case, p, Om=None, mu=None, fast=False):
    """{nt: (draws (K, C, nt, P), stats (K, C, 8))} for nt = 1, 2, 3 at the cavities (Om, mu) (default: the nominal
    ones), from the strict oracle build or the fast one."""
    Om = p['Oms'] if Om is None else Om
    mu = p['mus'] if mu is None else mu

    def run():
        return {nt: no.nuts_transitions(case.shape.model, p['X'], p['y'], p['k_lim'], mu, Om, SEEDS, p['q0'], p['eps'],
                                        p['inv_e'], nt=nt, t_offset=T_OFFSET, g_cnt=p['g_cnt'], g_lim=p['g_lim'])
                for nt in range(1, NT + 1)}
    if fast:
        with no.timing_build():
            return run()
    return run()


def per_transition(runs, whole=True):
    """From the runs of nt = 1, 2, 3 transitions (the hook keeps no trace: epx_set_trace is off when step sizes are
    injected): leapfrogs, divergences, depth and accept statistic of each transition, (K, C, NT) each.  A run of nt
    transitions repeats the first nt - 1 of the longer ones (same stream, same start), so the differences of the sums
    are the transitions' own figures.  whole: the counts must come out as whole numbers (an oracle run's do)."""
    out = {}
    for name, idx, mean in (('leapfrogs', 2, False), ('divergent', 4, False), ('depth', 6, True), ('accept', 5, True)):
        tot = np.stack([runs[nt][1][:, :, idx] * (nt if mean else 1) for nt in range(1, NT + 1)], axis=2)
        out[name] = np.diff(np.concatenate([np.zeros_like(tot[:, :, :1]), tot], axis=2), axis=2)
    for name in ('leapfrogs', 'divergent', 'depth'):
        r = np.rint(out[name])
        assert not whole or np.abs(out[name] - r).max() < 1e-9, (name, out[name])
        out[name] = r.astype(np.int64)
    return out


def site_rows(p, k):
    """Rows of site k and its groups' row limits relative to the site's first row (None: one group)."""
    lo, hi = int(p['k_lim'][k]), int(p['k_lim'][k + 1])
    gl = None
    if p['g_cnt'] is not None:
        off = np.concatenate(([0], np.cumsum(p['g_cnt'])))
        gl = p['g_lim'][off[k]:off[k + 1] + 1] - lo
    return lo, hi, gl


def first_leaf(case, p, k, c, Om=None, mu=None):
    """(log density, gradient) of the oracle's `logdensity_grad` at the first leaf of chain (k, c)'s first transition:
    the momentum and the direction from the shared random stream (kinds 1 and 2 of the probe), one leapfrog from q0."""
    Om = p['Oms'] if Om is None else Om
    mu = p['mus'] if mu is None else mu
    model = case.shape.model
    lo, hi, gl = site_rows(p, k)
    Pk = no.dims(model, case.shape.D, 1 if gl is None else len(gl) - 1)[1]
    t = T_OFFSET + 1
    z = np.array([no.rng_probe(int(SEEDS[k]), c, t, 1, a, 0)[2:] for a in range((Pk + 1) // 2)]).ravel()[:Pk]
    inv_e, q0 = p['inv_e'][k, c, :Pk], p['q0'][k, c, :Pk]
    mom = z / np.sqrt(inv_e)
    eps = p['eps'][k, c] * (1.0 if no.rng_probe(int(SEEDS[k]), c, t, 2, 0, 0)[0] > 0.5 else -1.0)
    X, y = p['X'][lo:hi], p['y'][lo:hi]
    _, g0 = no.logdensity_grad(model, X, y, mu[k], Om[k], q0, gl=gl)
    with np.errstate(all='ignore'):
        q1 = q0 + eps * inv_e * (mom + 0.5 * eps * g0)
    return no.logdensity_grad(model, X, y, mu[k], Om[k], q1, gl=gl)


def check_claims(case, p, per, Om=None, mu=None):
    """Every chain of the case has the ending it claims (assertions on an oracle run's per-transition figures)."""
    lf, dv, dp = per['leapfrogs'], per['divergent'], per['depth']
    for k in range(p['K']):
        for c in range(p['C']):
            ctx = (case.id, k, c, lf[k, c], dv[k, c], dp[k, c])
            for kind in case.claims[k][c]:
                if kind == 'cap':
                    assert np.all(lf[k, c] == CAP_LEAPFROGS) and np.all(dp[k, c] == 10) and np.all(dv[k, c] == 0), ctx
                elif kind == 'first_leaf':
                    assert np.all(lf[k, c] == 1) and np.all(dp[k, c] == 0) and np.all(dv[k, c] == 1), ctx
                elif kind == 'mid_tree':
                    assert dv[k, c, 0] == 1 and lf[k, c, 0] >= 3, ctx
                elif kind == 'nonfinite':
                    lp, g = first_leaf(case, p, k, c, Om, mu)
                    assert not (np.isfinite(lp) and np.all(np.isfinite(g))), ctx + (lp,)
                elif kind == 'uturn':
                    assert dv[k, c, 0] == 0 and lf[k, c, 0] < CAP_LEAPFROGS, ctx
                else:
                    raise AssertionError('unknown kind %r' % (kind,))


# ---------------------------------------------------------------- max_treedepth below 10: whole short runs
# Full site updates (warm-up included) at a reduced cap, compared with the oracle's trace transition by transition.
# A dominant cavity: the chains stay with the oracle for most of the run, and a quarter of the transitions ends below
# the cap (U-turn or divergence) beside the ones that reach it.  Depths per shape (STACK_PLAN):
#   (16, 48) and (40, 48): 1 (a tree is one leaf), 3 and 4 -- no boundary of the stack lies there (wholly in LDS for
#       layouts 1 2 5 6 7, wholly global for 3): the cap itself is what is compared;
#   (32, 500): 2, 3, 4 -- layout 7's stack is whole in LDS at 2, split with every level in LDS at 3, and reaches the
#       global store at 4; layouts 5 and 1 run all three from the global store.
DEPTH_RUN = dict(model='m4b_sg', K=2, chains=4, iter=30, tight=1000.0, seed=41,
                 shapes=(((16, 48), (1, 2, 5, 6, 7), (1, 3, 4)), ((40, 48), (3,), (1, 3, 4)), ((32, 500), (7, 5, 1), (2, 3, 4))))


def depth_run_problem(D, n):
    r = DEPTH_RUN
    X, y, k_lim, Oms, mus, d, P = _site_problem(r['model'], D, n, r['seed'], K=r['K'], tight=r['tight'])
    seeds = np.arange(r['K'], dtype=np.int64) * 7 + 3 + r['seed']
    return X, y, k_lim, Oms, mus, P, seeds


def at_cap(trace, max_depth):
    """Transitions of a trace (..., 8 + P) that ended at the cap: depth max_depth, 2^max_depth - 1 leapfrogs."""
    return (trace[..., 1] == 2 ** max_depth - 1) & (trace[..., 3] == max_depth) & (trace[..., 4] == 0)
