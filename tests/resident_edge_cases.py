"""The case table of the resident samplers' edge tests (plain helper, no tests): test_resident_edge_cases.py (no device)
and test_gpu_resident_edges.py (device) share it.

The resident kernels (csrc/nuts.hip k_nuts and k_nuts_spec, csrc/nuts_duo.hip, with csrc/nuts_gradient.inc and
csrc/nuts_gradient_groups.inc) are compiled once per (NV, DP) and per home of the cavity precision, the tree stack and
the bookkeeping wave's records; which instantiation a site runs is decided by the LDS its rows leave
(nuts_lds_layout, nuts_duo_lds_layout) in the order csrc/epx_api.hip plan_sampler tries the forms.  `plan` below restates
that order ONCE, over the library's own layout functions (tests/resident_plan_probe.hip):

    DP   = 4 | 8 | 16 | 32, the first that holds D            columns of a resident row (the columns beyond D are zeros)
    NV   = ceil(P / 64)                                       registers per chain vector
    family   one1 / one4    k_nuts, WPC = 1 (layout 1) or 4 (layout 2 without room for the bookkeeping wave's records)
             spec           k_nuts_spec, the cavity precision and stack in LDS (RES) or both in global memory
             spec-grp       k_nuts_spec for several groups per site
             duo41 / duo44 / duo12    k_nuts_duo (CPB, RW): layouts 5, 7, 6
             stream         no resident form takes the shape: layout 3

Every case states, as literal numbers, the served layout, (d, P, DP, NV) and the claim (family, om_in_lds, stack_in_lds,
stack_lds_levels, off_spec > 0, npad, tail columns, team_tiles_per_wave) of the launch its check makes: the gradient hook
plans ONE chain, the transition hook four, so a case belongs to one of the two (`chains`).  The CPU test holds every
claim against the oracle's dimensions and `plan` over the probe.  Parts, as the device test runs them:

    H  homes: per resident layout and model, a site one row below and one at every boundary where the planner moves the
       precision, the stack or the bookkeeping records out of LDS, or serves another layout; transitions across the
       boundaries where the stack's home changes;
    I  one gradient case per reachable instantiation (family, NV, DP, GAUSS) that no earlier device test compares with a
       reference (existing_launches / COVERED below), and one transition case per family;
    C  columns: both sides of every DP switch, one padding column, and the shapes with P in 63 .. 66, d in 62 .. 66 where
       an element of the chain rule lands in the second register and the cavity tail holds zero, one and two columns;
    R  rows: 1, 63, 64, 65 (layout 1), 1, 255, 256, 257 (layouts 2, 6), a one-row site beside the largest the layout holds,
       and the longest product of factors a lane of layout 1 forms at DP = 4 (theta = 0: every factor exactly 2);
    N  a site's bits unchanged when its neighbour's rows are multiplied by 1e300 and when they are NaN.

Where transitions are compared the cavity is a dominant one (tight = 1000) and start points, step sizes and metric come
from the ORACLE's own 24-iteration run: nothing here depends on the device.  A case at which the strict and the fast
oracle build part gets another seed (`seed`), never a looser bound on the device."""

import subprocess

import numpy as np

from oracle import nuts_oracle as no
from test_gpu_parity import _group_problem, _site_problem

LDS_CAP = 160 * 1024
TIGHT = 1000.0
ITER = 24
T_OFFSET = 4
MAX_DEPTH = 10            # what epx_logdensity_grad_layout and epx_nuts_transitions plan with
MAX_FACTORS = 80          # csrc/nuts_gradient.inc: a lane's running product takes at most 80 factors of at most 2^12
NEIGHBOUR_SCALE = 1e300


def pad_dp(D):
    """csrc/epx_api.hip pad_dp."""
    return 4 if D <= 4 else 8 if D <= 8 else 16 if D <= 16 else 32 if D <= 32 else -1


class Probe:
    """nuts_lds_layout / nuts_duo_lds_layout through tests/resident_plan_probe.hip, cached."""
    FIELDS = ('om', 'st', 'lv', 'off_spec', 'tail_bytes', 'lds_bytes', 'ret', 'has', 'tpw', 'npad', 'tail')

    def __init__(self, exe):
        self.exe, self.cache = exe, {}

    def many(self, tuples):
        todo = [t for t in dict.fromkeys(tuples) if t not in self.cache]
        if todo:
            out = subprocess.run([self.exe, 'plan'], input='\n'.join(' '.join(str(x) for x in t) for t in todo) + '\n',
                                 stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout.splitlines()
            assert len(out) == len(todo)
            for t, line in zip(todo, out):
                self.cache[t] = dict(zip(self.FIELDS, (int(x) for x in line.split())))
        return [self.cache[t] for t in tuples]

    def __call__(self, form, wpc, cpb, rw, grp, ngmax, gauss, P, d, dp, n_max, md):
        return self.many([(form, wpc, cpb, rw, grp, ngmax, gauss, P, d, dp, n_max, md)])[0]


def forms(P, d, dp, gauss, n_max, chains, md=MAX_DEPTH):
    """The probe tuples `plan` can ask for at a single-group shape (to fill the cache in one call)."""
    return [(f[0], f[1], f[2], f[3], 0, 0, int(gauss), P, d, dp, n_max, md)
            for f in ((0, 1, min(chains, 4), 0), (0, 4, 1, 0), (1, 0, 4, 1), (1, 0, 4, 4), (1, 0, 1, 2))]


def plan(lay, D, d, P, n_max, gauss, multi=False, ngmax=0, layout=0, chains=4, max_depth=MAX_DEPTH, no_spec=0):
    """csrc/epx_api.hip plan_sampler restated for the RESIDENT forms of a launch of fewer than 192 sites, in its order of
    attempts; `lay` is the library's layout function (Probe).  Returns dict(served, fam, nv, dp, gauss, om, st, lv, spec,
    npad, tail, tpw, lds_bytes); served 3 (fam 'stream') where no resident form takes the shape.  Layout 0 only for the
    Gaussian family, layout 4 not at all (the streaming table's)."""
    nv, dp = (P + 63) // 64, pad_dp(D)
    assert layout in (1, 2, 5, 6, 7) or (layout == 0 and gauss)
    out = dict(nv=nv, dp=dp, gauss=int(gauss), lv=0, npad=0, tail=0, tpw=0)

    def done(served, fam, r, **kw):
        out.update(served=served, fam=fam, om=r['om'], st=r['st'], spec=int(r['off_spec'] > 0), lds_bytes=r['lds_bytes'], **kw)
        return out

    stream = dict(om=0, st=0, off_spec=0, lds_bytes=-1)
    if multi:
        # several groups per site: the everything-resident bookkeeping-wave kernel, or the lock-step layouts 4 / 3
        if dp > 0 and nv <= 2 and not no_spec and layout in (2, 0):
            r = lay(0, 4, 1, 0, 1, ngmax, int(gauss), P, d, dp, n_max, max_depth)
            if r['ret'] <= LDS_CAP and r['om'] and r['st'] and r['off_spec'] > 0:
                return done(2, 'spec-grp', r)
        return done(3, 'stream', stream)
    if not gauss and dp > 0 and nv <= 2 and not no_spec and layout in (5, 6, 7):
        for cand in ((6,) if layout == 6 else (5,) if layout == 5 else (7, 5)):       # (a request for 7 that does not fit: 5)
            cpb, rw = (1, 2) if cand == 6 else (4, 4) if cand == 7 else (4, 1)
            r = lay(1, 0, cpb, rw, 0, 0, 0, P, d, dp, n_max, max_depth)
            fits = (r['has'] and r['ret'] <= LDS_CAP and
                    ((n_max + 63) // 64 <= 32 if cand == 7 else (n_max + 64 * rw - 1) // (64 * rw) <= 64) and (cand != 6 or r['st']))
            if fits:
                return done(cand, 'duo%d%d' % (cpb, rw), r, lv=r['lv'], npad=r['npad'], tail=r['tail'], tpw=r['tpw'])
    if layout in (0, 5, 6, 7):
        layout = 2                                               # (fewer sites than fill the chip)
    resident = dp > 0 and nv <= 2
    if resident:
        wpc, cpb = (1, min(chains, 4)) if layout == 1 else (4, 1)
        r = lay(0, wpc, cpb, 0, 0, 0, int(gauss), P, d, dp, n_max, max_depth)
        resident = r['ret'] <= LDS_CAP
        if gauss and resident:                                   # the Gaussian family: its everything-in-LDS forms only
            resident = bool(r['om'] and (wpc == 1 or (r['st'] and r['off_spec'] > 0 and not no_spec)))
    if not resident:
        return done(3, 'stream', stream)
    if wpc == 4 and r['off_spec'] > 0 and not no_spec:           # csrc/nuts.hip launch_wpc
        return done(2, 'spec', r)
    if wpc == 4:
        both = int(r['om'] and r['st'])                          # (both homes in LDS, or the kernel of neither)
        return done(2, 'one4', dict(r, om=both, st=both))
    return done(1, 'one1', r)


def sweep(lay, model, D, req, chains):
    """The plan of every site size from one row to beyond the LDS: (plans, indexed by n; the n at which (served layout,
    claim) differs from n - 1)."""
    d, P = no.dims(model, D)
    g, dp = no.is_gauss(model), pad_dp(D)
    top = LDS_CAP // (dp * 8) + 3
    lay.many([t for n in range(1, top) for t in forms(P, d, dp, g, n, chains)])
    plans = [None] + [plan(lay, D, d, P, n, g, layout=req, chains=chains) for n in range(1, top)]
    key = lambda r: (r['served'],) + claim_of(r)[:5]
    return plans, [n for n in range(2, top) if key(plans[n]) != key(plans[n - 1])]


CLAIM_KEYS = ('fam', 'om', 'st', 'lv', 'spec', 'npad', 'tail', 'tpw')


def claim_of(r):
    return tuple(r[k] for k in CLAIM_KEYS)


def instantiation(r):
    """(family, NV, DP, GAUSS): what launch_wpc / launch_duo_shape instantiate apart from the homes (part H's)."""
    fam = r['fam']
    if fam == 'spec':
        fam = 'spec-res' if r['om'] else 'spec-nonres'
    return (fam, r['nv'], r['dp'], r['gauss'])


SG_B = ('m1b_sg', 'm2b_sg', 'm3b_sg', 'm4b_sg', 'm5b_sg')
SG_A = ('m1a_sg', 'm2a_sg', 'm3a_sg', 'm4a_sg', 'm5a_sg')
MULTI = ('m1b', 'm2b', 'm3b', 'm4b', 'm5b', 'm1a', 'm2a', 'm3a', 'm4a', 'm5a')
REACH_GRID = 96


def reachable(lay):
    """Every instantiation some site of the model family reaches: all models, D = 1 .. 32, REACH_GRID site sizes up to
    the LDS, every request (layout 2 also with flags = 1, as sample_batch takes it); several groups: 2 .. 40 per site."""
    got = set()
    for model in SG_B + SG_A:
        g = no.is_gauss(model)
        reqs = ((1, 0), (2, 0), (0, 0)) if g else ((1, 0), (2, 0), (2, 1), (5, 0), (6, 0), (7, 0))
        for D in range(1, 33):
            d, P = no.dims(model, D)
            dp = pad_dp(D)
            top = LDS_CAP // (dp * 8) + 2
            ns = sorted({1 + (top - 1) * i // REACH_GRID for i in range(REACH_GRID + 1)})
            lay.many([t for n in ns for t in forms(P, d, dp, g, n, 1)])
            for n in ns:
                for req, flag in reqs:
                    r = plan(lay, D, d, P, n, g, layout=req, chains=1, no_spec=flag)
                    if r['served'] != 3:
                        got.add(instantiation(r))
    shapes = [(model, D, ng) + no.dims(model, D, ng) for model in MULTI for D in range(1, 33) for ng in range(2, 41)]
    shapes = [s for s in shapes if s[4] <= 128]
    lay.many([(0, 4, 1, 0, 1, ng, int(no.is_gauss(model)), P, d, pad_dp(D), 2 * ng, MAX_DEPTH) for model, D, ng, d, P in shapes])
    for model, D, ng, d, P in shapes:
        r = plan(lay, D, d, P, 2 * ng, no.is_gauss(model), multi=True, ngmax=ng, layout=2)
        if r['served'] == 2:
            got.add(instantiation(r))
    return got


# ---------------------------------------------------------------- what the earlier device tests compare with a reference
def _gauss_layouts(D, n, d, P):
    """test_logdensity_gradient_matches_oracle's own choice of layouts for the Gaussian family."""
    dp = [c for c in (4, 8, 16, 32) if c >= D][0]
    lds1 = n * dp * 8 + n * 8 + d * d * 8
    nv = (P + 63) // 64
    lds2 = lds1 + 2 * 4 * (64 * (1 + nv) + 2) * 8 + 10 * (4 * nv * 64 + 2) * 8 + 2 * (7 * nv * 64 + 72) * 8
    return (0,) if lds1 > LDS_CAP else (1,) if lds2 > LDS_CAP else (2, 1)


def existing_launches():
    """(test, model, D, rows of the largest site, groups of the largest site or 0, chains, requested layout) of every
    launch of a resident layout that an earlier device test compares with the oracle or with layout 1."""
    out = []
    t = 'test_gpu_parity::test_logdensity_gradient_matches_oracle'
    for model in SG_B + SG_A:
        for D, n in ((3, 7), (4, 50), (16, 200), (21, 333), (32, 500)):
            for req in (_gauss_layouts(D, n, *no.dims(model, D)) if no.is_gauss(model) else (2, 1)):
                out.append((t, model, D, n, 0, 1, req))
    t = 'test_gpu_lean_math::test_logdensity_gradient_at_saturated_logits'
    for model in ('m1b_sg', 'm4b_sg', 'm2b_sg', 'm3b_sg', 'm5b_sg'):
        for D, n in ((4, 50), (32, 65), (16, 200)) if model in ('m1b_sg', 'm4b_sg') else ((16, 200),):
            for req in (1, 2, 5, 6, 7):
                out.append((t, model, 9 if (D == 4 and req >= 5) else D, n, 0, 1, req))
    t = 'test_gpu_round2::test_duo_gradients_match_oracle'
    for model, D, n in (('m4b_sg', 16, 200), ('m4b_sg', 32, 500), ('m1b_sg', 32, 300), ('m5b_sg', 21, 333), ('m3b_sg', 11, 64),
                        ('m2b_sg', 32, 100)):
        out += [(t, model, D, n, 0, 1, req) for req in (5, 6)]
    t = 'test_gpu_parity::test_multigroup_gradient_matches_oracle'
    for model in ('m1b', 'm2b', 'm3b', 'm4b', 'm5b'):
        for D, n, ng in ((3, 15, 3), (16, 50, 3), (40, 55, 2), (70, 65, 3)):
            out.append((t, model, D, n, ng, 1, 2))
    t = 'test_gpu_team_invariants'
    for D, n in ((32, 500), (32, 512), (32, 33), (32, 129), (32, 65), (16, 200)):
        out += [(t, 'm4b_sg', D, n, 0, ch, req) for ch in (1, 4) for req in (1, 7)]
    t = 'test_gpu_tree_endings::test_layout_ends_trees_as_the_oracle_does'
    out += [(t, 'm4b_sg', 16, 48, 0, 4, req) for req in (1, 2, 5, 6, 7)] + [(t, 'm4b_sg', 16, 48, 0, 3, 7)]
    out += [(t, 'm1b_sg', 16, 48, 0, 4, req) for req in (1, 7)] + [(t, 'm4a_sg', 16, 48, 0, 4, req) for req in (1, 2)]
    out += [(t, 'm4b', 4, 50, 3, 4, 2)] + [(t, 'm4b_sg', 32, 500, 0, 4, req) for req in (7, 5, 1)]
    t = 'test_gpu_parity::test_ragged_sites_and_extreme_shapes'
    out += [(t, model, D, n, 0, 1, 2) for model, D, n in (('m1b_sg', 1, 700), ('m4b_sg', 5, 1500), ('m3b_sg', 32, 300), ('m2b_sg', 7, 512))]
    return out


def covered_by_existing(lay):
    """instantiation -> the first test of existing_launches that runs it."""
    got = {}
    for test, model, D, n, ng, chains, req in existing_launches():
        d, P = no.dims(model, D, max(ng, 1))
        if pad_dp(D) < 0 or P > 128:
            continue                                             # (streamed: not a resident kernel)
        r = plan(lay, D, d, P, n, no.is_gauss(model), multi=ng > 0, ngmax=ng, layout=req, chains=chains)
        if r['served'] != 3:
            got.setdefault(instantiation(r), test)
    return got


# The committed coverage list: every instantiation an earlier device test compares with a reference, and that test
# (test_resident_edge_cases.py recomputes it from existing_launches over the library's planning).  Part I is the
# complement within `reachable`.
_T = {'par': 'test_gpu_parity::test_logdensity_gradient_matches_oracle',
      'sat': 'test_gpu_lean_math::test_logdensity_gradient_at_saturated_logits',
      'duo': 'test_gpu_round2::test_duo_gradients_match_oracle',
      'grp': 'test_gpu_parity::test_multigroup_gradient_matches_oracle',
      'rag': 'test_gpu_parity::test_ragged_sites_and_extreme_shapes'}
COVERED = {
    ('duo12', 1, 16, 0): _T['sat'], ('duo12', 1, 32, 0): _T['sat'], ('duo12', 2, 32, 0): _T['sat'],
    ('duo41', 1, 16, 0): _T['sat'], ('duo41', 1, 32, 0): _T['sat'], ('duo41', 2, 32, 0): _T['sat'],
    ('duo44', 1, 16, 0): _T['sat'], ('duo44', 1, 32, 0): _T['sat'], ('duo44', 2, 32, 0): _T['sat'],
    ('one1', 1, 4, 0): _T['par'], ('one1', 1, 4, 1): _T['par'], ('one1', 1, 16, 0): _T['par'], ('one1', 1, 16, 1): _T['par'],
    ('one1', 1, 32, 0): _T['par'], ('one1', 1, 32, 1): _T['par'], ('one1', 2, 32, 0): _T['par'], ('one1', 2, 32, 1): _T['par'],
    ('one4', 1, 32, 0): _T['par'],                   # (m1b_sg at (32, 500): in the band without room for the bookkeeping records)
    ('spec-grp', 1, 4, 0): _T['grp'], ('spec-grp', 1, 16, 0): _T['grp'], ('spec-grp', 2, 16, 0): _T['grp'],
    ('spec-nonres', 2, 32, 0): _T['par'],            # (m4b_sg at (32, 500))
    ('spec-res', 1, 4, 0): _T['par'], ('spec-res', 1, 4, 1): _T['par'], ('spec-res', 1, 8, 0): _T['rag'],
    ('spec-res', 1, 16, 0): _T['par'], ('spec-res', 1, 16, 1): _T['par'], ('spec-res', 1, 32, 0): _T['par'],
    ('spec-res', 1, 32, 1): _T['par'], ('spec-res', 2, 32, 0): _T['par'],
}


class Case:
    """One engine's worth of sites.  sites: rows per site (a `_sg` model) or the list of group sizes per site.
    geo: (d, P, DP, NV).  claim: CLAIM_KEYS of the launch the check makes with `chains` chains (1: the gradient hook,
    4: the transition hook).  checks: 'grad', 'trans', 'neighbour'."""

    def __init__(self, part, model, D, sites, req, served, geo, claim, checks=('grad',), chains=1, tight=1.0, seed=None,
                 eps_scale=1.0, note=''):
        self.part, self.model, self.D, self.sites, self.req, self.served = part, model, D, list(sites), req, served
        self.d, self.P, self.dp, self.nv = geo
        self.claim, self.checks, self.chains, self.tight, self.eps_scale, self.note = tuple(claim), tuple(checks), chains, tight, eps_scale, note
        self.multi = not model.endswith('_sg')
        self.K = len(self.sites)
        self.rows = [sum(s) if self.multi else s for s in self.sites]
        self.n_max = max(self.rows)
        self.ngmax = max(len(s) for s in self.sites) if self.multi else 0
        self.gauss = no.is_gauss(model)
        self.seed = 900 + D + self.n_max if seed is None else seed
        self.id = '%s-%s-D%d-%s-L%d-c%d' % (part, model, D, '+'.join('%dg%d' % (len(s), sum(s)) if self.multi else 'n%d' % s
                                                                     for s in self.sites), req, chains)
        self.compared = 'trans' in self.checks
        self.shape = (model, D, repr(self.sites), tight, self.seed, self.compared, eps_scale)     # (cases that share their inputs)

    def __repr__(self):
        return self.id

    def plan(self, lay):
        return plan(lay, self.D, self.d, self.P, self.n_max, self.gauss, multi=self.multi, ngmax=self.ngmax, layout=self.req,
                    chains=self.chains)


CASES = []


def _c(*a, **kw):
    CASES.append(Case(*a, **kw))


_T4 = dict(checks=('trans',), chains=4, tight=TIGHT)

# the claims, CLAIM_KEYS order: (family, om_in_lds, stack_in_lds, stack_lds_levels, off_spec > 0, npad, tail columns, tiles per wave)
W1_BOTH, W1_OM, W1_NONE = ('one1', 1, 1, 0, 0, 0, 0, 0), ('one1', 1, 0, 0, 0, 0, 0, 0), ('one1', 0, 0, 0, 0, 0, 0, 0)
W4_RES, W4_GLB = ('one4', 1, 1, 0, 0, 0, 0, 0), ('one4', 0, 0, 0, 0, 0, 0, 0)
S_RES, S_GLB, S_GRP = ('spec', 1, 1, 0, 1, 0, 0, 0), ('spec', 0, 0, 0, 1, 0, 0, 0), ('spec-grp', 1, 1, 0, 1, 0, 0, 0)
STREAM = ('stream', 0, 0, 0, 0, 0, 0, 0)


def d41(st, npad, tail):
    return ('duo41', 1, st, 0, 0, npad, tail, 0)


def d12(npad, tail):
    return ('duo12', 1, 1, 0, 1, npad, tail, 0)


def d44(st, lv, tail, tpw):
    return ('duo44', 1, st, lv, 0, 0, tail, tpw)


# ---------------------------------------------------------------- H: homes
# Per (model, requested layout): (rows, served layout, claim), in pairs one row below and at every row count where the
# plan of a ONE-chain launch (the gradient hook) changes -- test_resident_edge_cases.py finds the same row counts by
# sweeping the library's planning.  D = 32: m4b_sg (d, P) = (66, 99), NV = 2, npad 32, two tail columns; m1b_sg (33, 34),
# NV = 1, npad 24; m4a_sg (67, 100), NV = 2.
H_GEO = {'m4b_sg': (66, 99, 32, 2), 'm1b_sg': (33, 34, 32, 1), 'm4a_sg': (67, 100, 32, 2)}
H_GRAD = {
    ('m4b_sg', 1): [(422, 1, W1_BOTH), (423, 1, W1_OM), (501, 1, W1_OM), (502, 1, W1_NONE), (637, 1, W1_NONE), (638, 3, STREAM)],
    ('m4b_sg', 2): [(313, 2, S_RES), (314, 2, W4_RES), (373, 2, W4_RES), (374, 2, S_GLB), (528, 2, S_GLB), (529, 2, W4_GLB),
                    (589, 2, W4_GLB), (590, 3, STREAM)],
    ('m4b_sg', 5): [(183, 5, d41(1, 32, 2)), (184, 5, d41(0, 32, 2)), (503, 5, d41(0, 32, 2)), (504, 2, S_GLB), (528, 2, S_GLB),
                    (529, 2, W4_GLB), (589, 2, W4_GLB), (590, 3, STREAM)],
    ('m4b_sg', 6): [(352, 6, d12(32, 2)), (353, 2, W4_RES), (373, 2, W4_RES), (374, 2, S_GLB), (528, 2, S_GLB), (529, 2, W4_GLB),
                    (589, 2, W4_GLB), (590, 3, STREAM)],
    ('m4b_sg', 7): [(256, 7, d44(1, 0, 2, 4)), (257, 7, d44(0, 4, 2, 6)), (384, 7, d44(0, 4, 2, 6)), (385, 7, d44(0, 3, 2, 8)),
                    (512, 7, d44(0, 3, 2, 8)), (513, 2, S_GLB), (528, 2, S_GLB), (529, 2, W4_GLB), (589, 2, W4_GLB), (590, 3, STREAM)],
    ('m1b_sg', 1): [(563, 1, W1_BOTH), (564, 1, W1_OM), (603, 1, W1_OM), (604, 1, W1_NONE), (637, 1, W1_NONE), (638, 3, STREAM)],
    ('m1b_sg', 2): [(498, 2, S_RES), (499, 2, W4_RES), (531, 2, W4_RES), (532, 2, S_GLB), (572, 2, S_GLB), (573, 2, W4_GLB),
                    (605, 2, W4_GLB), (606, 3, STREAM)],
    ('m1b_sg', 5): [(426, 5, d41(1, 24, 0)), (427, 5, d41(0, 24, 0)), (586, 5, d41(0, 24, 0)), (587, 2, W4_GLB), (605, 2, W4_GLB),
                    (606, 3, STREAM)],
    ('m1b_sg', 6): [(510, 6, d12(24, 0)), (511, 2, W4_RES), (531, 2, W4_RES), (532, 2, S_GLB), (572, 2, S_GLB), (573, 2, W4_GLB),
                    (605, 2, W4_GLB), (606, 3, STREAM)],
    ('m1b_sg', 7): [(384, 7, d44(1, 0, 0, 6)), (385, 7, d44(0, 4, 0, 8)), (512, 7, d44(0, 4, 0, 8)), (513, 5, d41(0, 24, 0)),
                    (586, 5, d41(0, 24, 0)), (587, 2, W4_GLB), (605, 2, W4_GLB), (606, 3, STREAM)],
    # the Gaussian family has the everything-in-LDS forms only: layout 2 (also as the default, 0) gives way to the
    # streaming kernel where the bookkeeping records stop fitting, layout 1 where the precision does
    ('m4a_sg', 0): [(301, 2, S_RES), (302, 3, STREAM)],
    ('m4a_sg', 1): [(406, 1, W1_BOTH), (407, 1, W1_OM), (484, 1, W1_OM), (485, 3, STREAM)],
    ('m4a_sg', 2): [(301, 2, S_RES), (302, 3, STREAM)],
}
# The same for a FOUR-chain launch (the transition hook), at the row counts where the tree stack leaves the LDS: two
# sites of one row below, two of the row count itself; layout 6 has no such form and is served by layout 2
H_TRANS = {
    ('m4b_sg', 1): [(183, 1, W1_BOTH), (184, 1, W1_OM)],
    ('m4b_sg', 2): [(373, 2, W4_RES), (374, 2, S_GLB)],
    ('m4b_sg', 5): [(183, 5, d41(1, 32, 2)), (184, 5, d41(0, 32, 2))],
    ('m4b_sg', 6): [(373, 2, W4_RES), (374, 2, S_GLB)],
    ('m4b_sg', 7): [(256, 7, d44(1, 0, 2, 4)), (257, 7, d44(0, 4, 2, 6))],
    ('m1b_sg', 1): [(444, 1, W1_BOTH), (445, 1, W1_OM)],
    ('m1b_sg', 2): [(531, 2, W4_RES), (532, 2, S_GLB)],
    ('m1b_sg', 5): [(426, 5, d41(1, 24, 0)), (427, 5, d41(0, 24, 0))],
    ('m1b_sg', 6): [(531, 2, W4_RES), (532, 2, S_GLB)],
    ('m1b_sg', 7): [(384, 7, d44(1, 0, 0, 6)), (385, 7, d44(0, 4, 0, 8))],
    ('m4a_sg', 1): [(174, 1, W1_BOTH), (175, 1, W1_OM)],
}
for (_m, _req), _rows in H_GRAD.items():
    for _n, _served, _claim in _rows:
        _c('H', _m, 32, [_n], _req, _served, H_GEO[_m], _claim)
for (_m, _req), _rows in H_TRANS.items():
    for _n, _served, _claim in _rows:
        _c('H', _m, 32, [_n, _n], _req, _served, H_GEO[_m], _claim, **_T4)

# ---------------------------------------------------------------- I: instantiations
# one gradient case per reachable (family, NV, DP, GAUSS) outside COVERED: the shapes are the smallest of their kind --
# k_nuts at WPC = 4 and the k_nuts_spec that keeps precision and stack in global memory exist only where the rows nearly
# fill the LDS, so their sites are long and narrow
_G11a, _G11b = [5, 1, 9, 4, 17, 3, 8, 2, 6, 1, 7], [4, 17, 3, 8, 2, 6, 1, 7, 11, 3, 5]
_c('I', 'm1b_sg', 7, [37, 37], 1, 1, (8, 9, 8, 1), W1_BOTH)
_c('I', 'm1a_sg', 7, [37, 37], 1, 1, (9, 10, 8, 1), W1_BOTH)
_c('I', 'm1b_sg', 3, [4150, 4150], 2, 2, (4, 5, 4, 1), W4_RES)
_c('I', 'm1b_sg', 7, [2103, 2103], 2, 2, (8, 9, 8, 1), W4_RES)
_c('I', 'm1b_sg', 13, [1053, 1053], 2, 2, (14, 15, 16, 1), W4_RES)
_c('I', 'm4b_sg', 29, [341, 341], 2, 2, (60, 90, 32, 2), W4_RES)
_c('I', 'm4a', 4, [[5, 1], [4, 17]], 2, 2, (11, 21, 4, 1), S_GRP)
_c('I', 'm4b', 7, [[5, 1], [4, 17]], 2, 2, (16, 32, 8, 1), S_GRP)
_c('I', 'm4a', 7, [[5, 1], [4, 17]], 2, 2, (17, 33, 8, 1), S_GRP)
_c('I', 'm4a', 13, [[5, 1], [4, 17]], 2, 2, (29, 57, 16, 1), S_GRP)
_c('I', 'm1b', 27, [[5, 1], [4, 17]], 2, 2, (28, 30, 32, 1), S_GRP)
_c('I', 'm1a', 27, [[5, 1], [4, 17]], 2, 2, (29, 31, 32, 1), S_GRP)
# the group kernel with two registers per chain vector at small D: eleven groups of m4b at D = 4 give P = 65
_c('I', 'm4b', 4, [_G11a, _G11b], 2, 2, (10, 65, 4, 2), S_GRP)
_c('I', 'm4a', 4, [_G11a, _G11b], 2, 2, (11, 66, 4, 2), S_GRP)
_c('I', 'm4b', 7, [_G11a[:7], _G11b[:7]], 2, 2, (16, 72, 8, 2), S_GRP)
_c('I', 'm4a', 7, [_G11a[:6], _G11b[:6]], 2, 2, (17, 65, 8, 2), S_GRP)
_c('I', 'm4a', 13, [[5, 1, 9], [4, 17, 3]], 2, 2, (29, 71, 16, 2), S_GRP)
_c('I', 'm4b', 27, [[5, 1], [4, 17]], 2, 2, (56, 112, 32, 2), S_GRP)
_c('I', 'm4a', 27, [[5, 1], [4, 17]], 2, 2, (57, 113, 32, 2), S_GRP)
_c('I', 'm1b_sg', 3, [4402, 4402], 2, 2, (4, 5, 4, 1), S_GLB)
_c('I', 'm1b_sg', 7, [2231, 2231], 2, 2, (8, 9, 8, 1), S_GLB)
_c('I', 'm1b_sg', 13, [1118, 1118], 2, 2, (14, 15, 16, 1), S_GLB)
_c('I', 'm1b_sg', 27, [544, 544], 2, 2, (28, 29, 32, 1), S_GLB)
_c('I', 'm1a_sg', 7, [37, 37], 2, 2, (9, 10, 8, 1), S_RES)
_c('I', 'm4a_sg', 29, [37, 37], 2, 2, (61, 91, 32, 2), S_RES)
# one transition case per family (four chains)
_c('I', 'm1b_sg', 13, [37, 37], 1, 1, (14, 15, 16, 1), W1_BOTH, **_T4)
_c('I', 'm1b_sg', 13, [37, 37], 2, 2, (14, 15, 16, 1), S_RES, **_T4)
_c('I', 'm1b_sg', 13, [37, 37], 5, 5, (14, 15, 16, 1), d41(1, 8, 0), **_T4)
_c('I', 'm1b_sg', 13, [37, 37], 7, 7, (14, 15, 16, 1), d44(1, 0, 0, 2), **_T4)
_c('I', 'm1b_sg', 13, [37, 37], 6, 6, (14, 15, 16, 1), d12(8, 0), **_T4)
_c('I', 'm1b_sg', 27, [512, 512], 2, 2, (28, 29, 32, 1), W4_RES, **_T4)
_c('I', 'm1b_sg', 27, [544, 544], 2, 2, (28, 29, 32, 1), S_GLB, **_T4)
_c('I', 'm4b', 4, [_G11a, _G11b], 2, 2, (10, 65, 4, 2), S_GRP, **_T4)
_c('I', 'm4b', 7, [_G11a[:7], _G11b[:7]], 2, 2, (16, 72, 8, 2), S_GRP, **_T4)

# ---------------------------------------------------------------- C: columns and vector registers
# two sites of 50 rows: everything is in LDS, the row team has two tiles per wave.  D -> (d, P, DP, NV, npad, tail columns)
C_N = 50
C_DP = {
    # both sides of every DP switch (4 | 5, 8 | 9, 16 | 17), one padding column (15, 31), nearly only padding (1, 2, 5, 9, 17)
    'm4b_sg': {1: (4, 6, 4, 1, 0, 0), 2: (6, 9, 4, 1, 0, 0), 4: (10, 15, 4, 1, 0, 0), 5: (12, 18, 8, 1, 0, 0), 8: (18, 27, 8, 1, 0, 0),
               9: (20, 30, 16, 1, 16, 0), 15: (32, 48, 16, 1, 16, 0), 16: (34, 51, 16, 1, 24, 0), 17: (36, 54, 32, 1, 24, 0),
               31: (64, 96, 32, 2, 32, 0), 32: (66, 99, 32, 2, 32, 2)},
    'm1b_sg': {1: (2, 3, 4, 1, 0, 0), 2: (3, 4, 4, 1, 0, 0), 4: (5, 6, 4, 1, 0, 0), 5: (6, 7, 8, 1, 0, 0), 8: (9, 10, 8, 1, 0, 0),
               9: (10, 11, 16, 1, 8, 0), 15: (16, 17, 16, 1, 8, 0), 16: (17, 18, 16, 1, 16, 0), 17: (18, 19, 32, 1, 16, 0),
               31: (32, 33, 32, 1, 16, 0), 32: (33, 34, 32, 1, 24, 0)},
}
# every shape of these models with P in 63 .. 66 or d in 62 .. 66 (m4b_sg D = 31: d = 64, NV = 2 with an EMPTY tail, and
# D = 32: d = 66, two tail columns, are in C_DP).  d = 65, the odd tail, exists in the Gaussian family only (m4a_sg D = 31),
# which has no row-wave kernels: k_nuts and k_nuts_spec run it, nuts_duo.hip cannot meet it.
C_REG = {
    'm4b_sg': {20: (42, 63, 32, 1, 24, 0), 21: (44, 66, 32, 2, 24, 0), 30: (62, 93, 32, 2, 32, 0)},
    'm3b_sg': {31: (32, 64, 32, 1, 16, 0), 32: (33, 66, 32, 2, 20, 0)},
    'm4a_sg': {20: (43, 64, 32, 1, 0, 0), 30: (63, 94, 32, 2, 0, 0), 31: (65, 97, 32, 2, 0, 0)},
    'm3a_sg': {30: (32, 63, 32, 1, 0, 0), 31: (33, 65, 32, 2, 0, 0)},
}


def _small(part, model, D, sites, geo6, reqs, tpw=2, **kw):
    """Sites that leave everything in LDS, per requested layout; layouts 5, 6, 7 have DP = 16 and 32 only and are served
    by layout 2 below that."""
    d, P, dp, nv, npad, tail = geo6
    for req in reqs:
        duo = req >= 5 and dp >= 16
        claim = {1: W1_BOTH, 2: S_RES, 5: d41(1, npad, tail), 6: d12(npad, tail), 7: d44(1, 0, tail, tpw)}[req] if duo or req < 5 else S_RES
        _c(part, model, D, sites, req, req if duo or req < 5 else 2, (d, P, dp, nv), claim, **kw)


for _part, _tab in (('C-dp', C_DP), ('C-reg', C_REG)):
    for _m, _by_D in _tab.items():
        for _D, _geo in _by_D.items():
            _small(_part, _m, _D, [C_N, C_N], _geo, (1, 2) + ((5, 6, 7) if _geo[2] >= 16 and not no.is_gauss(_m) else ()))
# d = 2: two of the four gradient waves of layout 2 get no column of the mat-vec
_small('C-d2', 'm2b_sg', 8, [C_N, C_N], (2, 11, 8, 1, 0, 0), (2,))

# ---------------------------------------------------------------- R: rows
_R_GEO = (34, 51, 16, 1, 24, 0)                        # m4b_sg, D = 16
for _n in (1, 63, 64, 65):                              # layout 1: a wave's lanes take rows lane, lane + 64, ...
    _small('R-rows', 'm4b_sg', 16, [_n, _n], _R_GEO, (1,))
for _n in (1, 255, 256, 257):                           # layouts 2 and 6: four and two waves share the rows
    _small('R-rows', 'm4b_sg', 16, [_n, _n], _R_GEO, (2, 6))
# a one-row site beside the largest site the layout still serves (H_GRAD): the LDS is laid out for the large one
_RAG = dict(checks=('grad', 'neighbour'))
_c('R-ragged', 'm4b_sg', 32, [1, 637], 1, 1, H_GEO['m4b_sg'], W1_NONE, **_RAG)
_c('R-ragged', 'm4b_sg', 32, [1, 589], 2, 2, H_GEO['m4b_sg'], W4_GLB, **_RAG)
_c('R-ragged', 'm4b_sg', 32, [1, 503], 5, 5, H_GEO['m4b_sg'], d41(0, 32, 2), **_RAG)
_c('R-ragged', 'm4b_sg', 32, [1, 352], 6, 6, H_GEO['m4b_sg'], d12(32, 2), **_RAG)
_c('R-ragged', 'm4b_sg', 32, [1, 512], 7, 7, H_GEO['m4b_sg'], d44(0, 3, 2, 8), **_RAG)
# DP = 4: the largest site layout 1 serves.  At theta = 0 every factor of a lane's product is exactly 2 and
# ceil(n / 64) = 78 of them multiply, under the 80 csrc/nuts_gradient.inc promises
FACTORS = dict(n=4964, factors=78)
_c('R-factors', 'm1b_sg', 4, [FACTORS['n']], 1, 1, (5, 6, 4, 1), W1_NONE)

# ---------------------------------------------------------------- N: neighbours
# site 0 with site 1's rows multiplied by 1e300, then NaN: the padding columns (D = 1: three of four, 5: three of eight,
# 17: fifteen of 32) and the rows behind the site's own must meet exact zeros
_N_GEO = {1: (4, 6, 4, 1, 0, 0), 5: (12, 18, 8, 1, 0, 0), 17: (36, 54, 32, 1, 24, 0)}
for _D in (1, 5, 17):
    _small('N', 'm4b_sg', _D, [C_N, C_N], _N_GEO[_D], (1, 2, 5, 7), checks=('neighbour',))


def cases(part=None, check=None):
    return [c for c in CASES if (part is None or c.part == part) and (check is None or check in c.checks)]


# ---------------------------------------------------------------- problems
_problems = {}


def problem(case):
    """The sites and their nominal cavities; for a `trans` case also q0 / eps / inv_e of the teacher-forced transitions
    from the oracle's own 24-iteration 4-chain run: the last kept draw, the adapted step size (times the case's
    eps_scale) and the site's pooled variance + 1e-6.  A ragged single-group engine takes the first rows of the equal
    sites _site_problem draws."""
    if case.shape in _problems:
        return _problems[case.shape]
    g_cnt = g_lim = None
    if case.multi:
        X, y, k_lim, g_cnt, g_lim, Oms, mus, d = _group_problem(case.model, case.D, case.sites, case.seed, tight=case.tight)
        P = no.dims(case.model, case.D, int(g_cnt.max()))[1]
        assert len(set(len(s) for s in case.sites)) == 1           # (every site has the engine's P coordinates)
    else:
        X, y, k_lim, Oms, mus, d, P = _site_problem(case.model, case.D, case.n_max, case.seed, K=case.K, tight=case.tight)
        k_lim = np.concatenate(([0], np.cumsum(case.rows)))
        X, y = X[:k_lim[-1]].copy(), y[:k_lim[-1]].copy()
    p = dict(X=X, y=y, k_lim=k_lim, g_cnt=g_cnt, g_lim=g_lim, Oms=Oms, mus=mus, d=d, P=P, K=case.K,
             seeds=np.arange(case.K, dtype=np.int64) + 21)
    if case.compared:
        draws, _, st = no.nuts_sites(case.model, X, y, k_lim, mus, Oms, p['seeds'], chains=4, iter=ITER, g_cnt=g_cnt, g_lim=g_lim)
        assert np.all(st[:, :, 7] == 0)
        p.update(q0=draws[:, :, -1, :].copy(), eps=st[:, :, 1] * case.eps_scale,
                 inv_e=np.repeat(draws.reshape(case.K, -1, P).var(axis=1)[:, None, :], 4, axis=1) + 1e-6)
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _problems[case.shape] = p
    return p


def site_rows(p, k):
    """Rows of site k and its groups' row limits relative to the site's first row (None: one group)."""
    lo, hi = int(p['k_lim'][k]), int(p['k_lim'][k + 1])
    gl = None
    if p['g_cnt'] is not None:
        off = np.concatenate(([0], np.cumsum(p['g_cnt'])))
        gl = p['g_lim'][off[k]:off[k + 1] + 1] - lo
    return lo, hi, gl


def thetas(case, p, k):
    """Two points per site: random at scale 0.5, and theta = 0."""
    rng = np.random.RandomState(6 + 10 * k + case.D)
    return [0.5 * rng.randn(p['P']), np.zeros(p['P'])]


def oracle_gradient(case, p, k, theta, Om=None, mu=None):
    Om = p['Oms'] if Om is None else Om
    mu = p['mus'] if mu is None else mu
    lo, hi, gl = site_rows(p, k)
    return no.logdensity_grad(case.model, p['X'][lo:hi], p['y'][lo:hi], mu[k], Om[k], theta, gl=gl)


def oracle_transitions(case, p, Om=None, mu=None, fast=False):
    """{nt: (draws (K, 4, nt, P), stats (K, 4, 8))} of nt = 1, 2, 3 teacher-forced transitions at the cavities (Om, mu)."""
    Om = p['Oms'] if Om is None else Om
    mu = p['mus'] if mu is None else mu

    def run():
        return {nt: no.nuts_transitions(case.model, p['X'], p['y'], p['k_lim'], mu, Om, p['seeds'], p['q0'], p['eps'], p['inv_e'],
                                        nt=nt, t_offset=T_OFFSET, g_cnt=p['g_cnt'], g_lim=p['g_lim']) for nt in (1, 2, 3)}
    if fast:
        with no.timing_build():
            return run()
    return run()


def depths(runs):
    """(K, 4, 3) tree depths of the three transitions from the mean depths of the nt = 1, 2, 3 runs."""
    tot = np.stack([nt * runs[nt][1][:, :, 6] for nt in (1, 2, 3)], axis=2)
    return np.rint(np.diff(np.concatenate((np.zeros_like(tot[:, :, :1]), tot), axis=2), axis=2)).astype(int)


def design_lines():
    """DESIGN.md's list of the reachable resident instantiations and the test that compares each with a reference."""
    part_i = {instantiation_of_claim(c): c.id for c in reversed(cases('I', 'grad'))}
    rows = dict(COVERED)
    rows.update({k: 'test_gpu_resident_edges::test_gradient_matches_oracle[%s]' % v for k, v in part_i.items()})
    return ['    %-11s NV = %d  DP = %-2d  %s  %s' % (k[0], k[1], k[2], 'Gaussian' if k[3] else 'logistic', rows[k]) for k in sorted(rows)]


def instantiation_of_claim(case):
    fam = case.claim[0]
    if fam == 'spec':
        fam = 'spec-res' if case.claim[1] else 'spec-nonres'
    return (fam, case.nv, case.dp, int(case.gauss))
