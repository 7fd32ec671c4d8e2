"""The case table of the streaming sampler's edge tests (plain helper, no tests): test_stream_edge_cases.py (no device)
and test_gpu_stream_edges.py (device) share it.

Layout 3 (csrc/nuts_stream.hip, csrc/epx_stream_tile.h) feeds a site's rows through a six-slot LDS-DMA ring of 16-row
tiles, three tiles in flight, the ring running on across leapfrog boundaries, and is compiled once per (DPB in
{64, 128}, NV = 1 .. 7, plain / pieced / looping).  What decides which code a site runs is written ONCE, here:

    DPB   = 64 if D <= 64 else 128          columns of a row image (columns D .. DPB - 1 read what follows the row)
    NV    = ceil(P / 64)                    registers per chain vector
    tiles = sum over groups of ceil(n_g / 16)   (a tile never straddles two groups)
    folds = tiles // 256                    how often the logistic wave folds its running product into a logarithm

Every case states the (d, P), DPB, NV, tiles per site, folds and ragged tiles it CLAIMS, as literal numbers; the CPU
test holds the claims against these formulas, against the oracle's own dimensions and against the library's LDS
planning (tests/stream_plan_probe.hip).  Parts, as the device test runs them:

    A  the gradient hook against the C oracle: tile counts 1 .. 7 (fewer tiles than the ring keeps in flight), the
       fold of the logistic wave's product (255 .. 1025 tiles), the column edges D = 63 64 65 127 and 1 2, and a site's
       independence of its neighbour's rows;
    B  every (DPB, NV) instantiation that no other test compares with a reference, as a sampler: gradient,
       teacher-forced transitions, a whole short run, and the pieced launch in both forms;
    C  one to three tiles over the hundreds of passes of a run (the ring's position moves by tiles mod 6 per pass);
    D  the tile table at the LDS limit (one tile below: served; at it: refused before any launch);
    E  the lock-step resident layout 4 at NV = 4 (its cold store).

Where transitions are compared the cavity is a dominant one (tight = 1000: short, non-chaotic trajectories), and the
start points, step sizes and metric of the teacher-forced transitions come from the ORACLE's own 24-iteration run:
nothing here depends on the device, so test_stream_edge_cases.py can hold the strict and the fast oracle build against
each other on exactly the inputs the device gets.  A case at which the two CPU builds part gets another seed (`seed`),
never a looser bound on the device."""

import numpy as np

from oracle import nuts_oracle as no
from test_gpu_parity import _group_problem, _site_problem

TR = 16                 # rows per tile (csrc/epx_stream_tile.h TR)
NSL = 6                 # ring slots (NSL)
RING_AHEAD = 3          # tiles in flight (EPX_RING_AHEAD)
FOLD_EVERY = 256        # stream_pass_impl: `if ((p & 255) == 0)`
TIGHT = 1000.0
ITER = 24               # whole short runs
NT = 3                  # teacher-forced transitions per launch
T_OFFSET = 4
LDS_PIECE_BYTES = 16    # csrc/epx_api.hip plan_sampler: the (site, first transition) words behind nuts_stream_lds_bytes


def dpb_of(D):
    return 64 if D <= 64 else 128


def nv_of(P):
    return -(-P // 64)


def tiles_of(groups):
    return sum(-(-n // TR) for n in groups)


def folds_of(tiles):
    return tiles // FOLD_EVERY


def ragged_of(groups):
    """[(tile index within the site, valid rows)] of the tiles that hold fewer than 16 rows."""
    out, t = [], 0
    for n in groups:
        t += -(-n // TR)
        if n % TR:
            out.append((t - 1, n % TR))
    return out


class Case:
    """One engine's worth of sites.  sites: per site the list of its groups' sizes (one entry: a `_sg` model).
    claims: d, P, dpb, nv, and per site tiles, folds, ragged.  checks: what the device test compares --
    'grad', 'trans' (teacher-forced), 'run' (a whole short run), 'pieces' (pieced launch = uncut launch),
    'resident' (layout 3 against layout 1 on the same engine).  layout: (requested, served)."""

    def __init__(self, part, model, D, sites, d, P, dpb, nv, tiles, folds, ragged, checks=('grad',), layout=(3, 3),
                 chains=4, tight=1.0, seed=None, note=''):
        self.part, self.model, self.D, self.sites = part, model, D, [list(s) for s in sites]
        self.d, self.P, self.dpb, self.nv = d, P, dpb, nv
        self.tiles, self.folds, self.ragged = list(tiles), list(folds), [list(r) for r in ragged]
        self.checks, self.layout, self.chains, self.tight, self.note = tuple(checks), layout, chains, tight, note
        self.multi = not model.endswith('_sg')
        self.K = len(self.sites)
        self.seed = 500 + D + sum(self.sites[0]) if seed is None else seed
        self.id = '%s-%s-D%d-%s-c%d' % (part, model, D, '+'.join('.'.join(str(n) for n in s) for s in self.sites)
                                        if self.multi else 'n%d' % self.sites[0][0], chains)
        self.compared = bool({'trans', 'run', 'pieces', 'resident'} & set(self.checks))

    def __repr__(self):
        return self.id


def _sg(part, model, D, n, d, P, dpb, nv, tiles, ragged, K=2, folds=0, **kw):
    """K single-group sites of n rows each."""
    return Case(part, model, D, [[n]] * K, d, P, dpb, nv, [tiles] * K, [folds] * K, [[ragged] if ragged else []] * K, **kw)


SAMPLER = ('grad', 'trans', 'run', 'pieces')

# n -> (tiles, the ragged tile as (index, rows) or None): one, two, three tiles are FEWER than the ring keeps in flight
# (ring_prime and the loader wrap t_i inside one pass: the same tile is in flight in several slots); 6 and 7 are the
# ring's own length and one more
TILE_COUNTS = {1: (1, (0, 1)), 15: (1, (0, 15)), 16: (1, None), 17: (2, (1, 1)), 32: (2, None), 33: (3, (2, 1)),
               96: (6, None), 97: (7, (6, 1))}

CASES = []

# ---------------------------------------------------------------- A: the gradient hook
for _n, (_t, _r) in sorted(TILE_COUNTS.items()):
    CASES.append(_sg('A-tiles', 'm1b_sg', 40, _n, 41, 42, 64, 1, _t, _r))
    CASES.append(_sg('A-tiles', 'm4a_sg', 40, _n, 83, 124, 64, 2, _t, _r, layout=(0, 3)))      # the Gaussian family's ragged yring

# the fold of the logistic wave's product: 255 tiles (no fold), 256 (the fold ON the last tile, which holds one row),
# 257; 513 and 1025 tiles (two and four folds: at theta = 0 every factor is exactly 2 and a lane's 1025 factors
# overflow a double without the fold)
CASES += [
    _sg('A-folds', 'm1b_sg', 33, 4080, 34, 35, 64, 1, 255, None, K=1),
    _sg('A-folds', 'm1b_sg', 33, 4081, 34, 35, 64, 1, 256, (255, 1), K=1, folds=1),
    _sg('A-folds', 'm1b_sg', 33, 4097, 34, 35, 64, 1, 257, (256, 1), K=1, folds=1),
    _sg('A-folds', 'm4b_sg', 8, 8200, 18, 27, 64, 1, 513, (512, 8), K=1, folds=2),
    _sg('A-folds', 'm4b_sg', 8, 16400, 18, 27, 64, 1, 1025, None, K=1, folds=4),
]
FOLD_ROW_SCALE = 30.0       # the same sites with their rows scaled: saturated logits

# column edges: DPB switches at D = 64 | 65; D = 63 and 127 leave one padding column, D = 1 and 2 nearly all of them
# D -> (d, P, DPB, NV)
for _model, _dims in (('m1b_sg', {63: (64, 65, 64, 2), 64: (65, 66, 64, 2), 65: (66, 67, 128, 2), 127: (128, 129, 128, 3),
                                  1: (2, 3, 64, 1), 2: (3, 4, 64, 1)}),
                      ('m4b_sg', {63: (128, 192, 64, 3), 64: (130, 195, 64, 4), 65: (132, 198, 128, 4), 127: (256, 384, 128, 6),
                                  1: (4, 6, 64, 1), 2: (6, 9, 64, 1)})):
    for _D in (63, 64, 65, 127, 1, 2):
        CASES.append(_sg('A-cols', _model, _D, 50, *_dims[_D], 4, (3, 2)))

# a site's result does not depend on its neighbour's rows: the padding columns of site 0's row images read site 1's
# rows (D = 1: 63 of 64 columns) and must meet exact zeros -- site 1's rows times NEIGHBOUR_SCALE change no bit
NEIGHBOUR_SCALE = 1e300
CASES += [
    _sg('A-neighbour', 'm1b_sg', 1, 50, 2, 3, 64, 1, 4, (3, 2)),
    _sg('A-neighbour', 'm4b_sg', 33, 50, 68, 102, 64, 2, 4, (3, 2)),
    _sg('A-neighbour', 'm1b_sg', 65, 50, 66, 67, 128, 2, 4, (3, 2)),
]

# ---------------------------------------------------------------- B: every vector width, as a sampler
_G5a, _G5b = [13, 20, 9, 17, 11], [16, 7, 25, 3, 19]          # 70 rows in 7 tiles each; the second site holds a full group


def _mg(part, D, d, P, nv, **kw):
    return Case(part, 'm4b', D, [_G5a, _G5b], d, P, 64 if D <= 64 else 128, nv, [7, 7], [0, 0],
                [[(0, 13), (2, 4), (3, 9), (5, 1), (6, 11)], [(1, 7), (3, 9), (4, 3), (6, 3)]], checks=SAMPLER, tight=TIGHT, **kw)


CASES += [
    _sg('B', 'm4b_sg', 63, 50, 128, 192, 64, 3, 4, (3, 2), checks=SAMPLER, tight=TIGHT, note='NV = 3 exactly full'),
    _sg('B', 'm4b_sg', 64, 70, 130, 195, 64, 4, 5, (4, 6), checks=SAMPLER, tight=TIGHT, chains=3, note='an idle chain slot'),
    _mg('B', 40, 82, 287, 5),
    _mg('B', 50, 102, 357, 6),
    _mg('B', 60, 122, 427, 7),
    _sg('B', 'm1b_sg', 127, 90, 128, 129, 128, 3, 6, (5, 10), checks=SAMPLER, tight=TIGHT),
    _sg('B', 'm4b_sg', 72, 45, 146, 219, 128, 4, 3, (2, 13), checks=SAMPLER, tight=TIGHT),
    # (seed: with the default one the two oracle builds end the six-chain run 1.1e-9 apart, above the table's 1e-9)
    _sg('B', 'm4b_sg', 85, 60, 172, 258, 128, 5, 4, (3, 12), checks=SAMPLER, tight=TIGHT, chains=6, seed=701,
        note='a second workgroup per site'),
    _sg('B', 'm3a_sg', 128, 75, 130, 259, 128, 5, 5, (4, 11), checks=SAMPLER, tight=TIGHT, layout=(0, 3)),
    _sg('B', 'm4b_sg', 127, 40, 256, 384, 128, 6, 3, (2, 8), checks=SAMPLER, tight=TIGHT, note='NV = 6 exactly full'),
]

# ---------------------------------------------------------------- C: few tiles over many passes
for _n in (1, 16, 17, 33):
    _t, _r = TILE_COUNTS[_n]
    CASES.append(_sg('C', 'm4b_sg', 40, _n, 82, 123, 64, 2, _t, _r, checks=('grad', 'trans', 'run'), tight=TIGHT))
    CASES.append(_sg('C', 'm4b_sg', 8, _n, 18, 27, 64, 1, _t, _r, checks=('grad', 'trans', 'run', 'resident'), tight=TIGHT))

# ---------------------------------------------------------------- D: the LDS limit
# m1b_sg, D = 8 (d = 9, P = 10, NV = 1, DPB = 64), layout 3 requested.  The tile table takes 8 bytes per tile; the first
# tile count the planner refuses is read from the library (test_stream_edge_cases.py: tests/stream_plan_probe.hip) and
# held against this figure, which is 160 KiB less everything else the kernel keeps in LDS, over 8 bytes.
LIMIT = dict(model='m1b_sg', D=8, d=9, P=10, dpb=64, nv=1, first_refused_tiles=12523)


def limit_problem(tiles, seed=77):
    """One site of 16 * tiles - 3 rows (its last tile ragged) and a small second site, nominal cavities."""
    n = TR * tiles - 3
    rng = np.random.RandomState(seed)
    D = LIMIT['D']
    X = rng.randn(n + 40, D)
    y = (rng.rand(n + 40) < 0.6).astype(int)
    d = LIMIT['d']
    Oms = np.stack([np.eye(d) * (1.0 + 0.5 * k) for k in range(2)])
    mus = 0.3 * rng.randn(2, d)
    return X, y, np.array([0, n, n + 40]), Oms, mus

# ---------------------------------------------------------------- E: lock-step resident layout at a wide vector
_G4a, _G4b = [23, 17, 40, 9], [16, 30, 5, 38]                  # 89 rows each, in 8 and in 7 tiles
CASES.append(Case('E', 'm4b', 32, [_G4a, _G4b], 66, 198, 32, 4, [8, 7], [0, 0],
                  [[(1, 7), (3, 1), (6, 8), (7, 9)], [(2, 14), (3, 5), (6, 6)]], checks=('grad', 'trans', 'run'),
                  layout=(4, 4), tight=TIGHT, note='layout 4: rows resident, DPB is the resident 32'))


def cases(part=None, check=None):
    return [c for c in CASES if (part is None or c.part == part) and (check is None or check in c.checks)]


# ---------------------------------------------------------------- problems
_problems = {}


def problem(case, row_scale=1.0):
    """The sites and their nominal cavities; for a compared case also q0 / eps / inv_e of the teacher-forced
    transitions from the oracle's own 24-iteration 4-chain run: the last kept draw, the adapted step size and the site's
    pooled variance + 1e-6.  row_scale: the same sites with every row scaled (part A's saturated logits)."""
    key = (case.id, row_scale)
    if key in _problems:
        return _problems[key]
    g_cnt = g_lim = None
    if case.multi:
        X, y, k_lim, g_cnt, g_lim, Oms, mus, d = _group_problem(case.model, case.D, case.sites, case.seed, tight=case.tight)
        P = no.dims(case.model, case.D, int(g_cnt.max()))[1]
    else:
        n = case.sites[0][0]
        assert all(s == [n] for s in case.sites)
        X, y, k_lim, Oms, mus, d, P = _site_problem(case.model, case.D, n, case.seed, K=case.K, tight=case.tight)
    if row_scale != 1.0:
        X = X * row_scale
    p = dict(X=X, y=y, k_lim=k_lim, g_cnt=g_cnt, g_lim=g_lim, Oms=Oms, mus=mus, d=d, P=P, K=case.K,
             seeds=np.arange(case.K, dtype=np.int64) + 21)
    if case.compared:
        draws, _, st = no.nuts_sites(case.model, X, y, k_lim, mus, Oms, p['seeds'], chains=4, iter=ITER, g_cnt=g_cnt, g_lim=g_lim)
        assert np.all(st[:, :, 7] == 0)
        p.update(q0=draws[:, :, -1, :].copy(), eps=st[:, :, 1].copy(),
                 inv_e=np.repeat(draws.reshape(case.K, -1, P).var(axis=1)[:, None, :], 4, axis=1) + 1e-6)
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _problems[key] = p
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
    """The points at which part A and the gradient checks of the other parts evaluate site k."""
    rng = np.random.RandomState(6 + 10 * k + case.D)
    if case.part == 'A-folds':
        return [np.zeros(p['P']), 0.5 * rng.randn(p['P'])]
    return [0.3 * rng.randn(p['P'])]


def oracle_gradient(case, p, k, theta, Om=None, mu=None):
    Om = p['Oms'] if Om is None else Om
    mu = p['mus'] if mu is None else mu
    lo, hi, gl = site_rows(p, k)
    return no.logdensity_grad(case.model, p['X'][lo:hi], p['y'][lo:hi], mu[k], Om[k], theta, gl=gl)


def oracle_transitions(case, p, Om=None, mu=None, fast=False):
    """(draws (K, 4, NT, P), stats (K, 4, 8)) of NT teacher-forced transitions at the cavities (Om, mu)."""
    Om = p['Oms'] if Om is None else Om
    mu = p['mus'] if mu is None else mu

    def run():
        return no.nuts_transitions(case.model, p['X'], p['y'], p['k_lim'], mu, Om, p['seeds'], p['q0'], p['eps'], p['inv_e'],
                                   nt=NT, t_offset=T_OFFSET, g_cnt=p['g_cnt'], g_lim=p['g_lim'])
    if fast:
        with no.timing_build():
            return run()
    return run()


def oracle_run(case, p, Om=None, mu=None, fast=False):
    """(draws (K, chains, ITER / 2, P), stats) of the whole short run with the case's chain count."""
    Om = p['Oms'] if Om is None else Om
    mu = p['mus'] if mu is None else mu

    def run():
        dr, _, st = no.nuts_sites(case.model, p['X'], p['y'], p['k_lim'], mu, Om, p['seeds'] + 10, chains=case.chains, iter=ITER,
                                  g_cnt=p['g_cnt'], g_lim=p['g_lim'])
        return dr, st
    if fast:
        with no.timing_build():
            return run()
    return run()
