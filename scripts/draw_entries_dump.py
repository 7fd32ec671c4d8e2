#!/usr/bin/env python3
"""Every array the entries over draws return, saved for a bit-for-bit comparison of two builds of libepx.so on one device:
HipEngine.named_moments, named_order_stats, pooled_count_pass, predict, loo, draw_diagnostics and pooled_moments at the
shapes of their tests/test_gpu_*.py files -- injected draws of single-group and multi-group models, and the sampler's own
draws of a short run (whole range and a sub-range) -- with fixed seeds; predict, loo, predict_new_group and
newgroup_latents at the edges of the predictive kernels' row-tile walk (tile_edges); and, at those edges and on the
multi-group engines, replicated_checks, site_evidence, predict_order_stats and draw_rank_diagnostics (later_entries).

    python scripts/draw_entries_dump.py --out a.npz                      # this tree's library
    EPX_LIB=/path/to/other/libepx.so python scripts/draw_entries_dump.py --out b.npz
    python scripts/draw_entries_dump.py --compare a.npz b.npz            # the same bytes in every array
"""

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 3, 9), (3, 4, 10), (21, 4, 25), (32, 4, 100), (128, 3, 11)]          # D, chains, draws per chain
GROUPS = [[9], [8, 7, 9], [10, 6]]


def problem(model, D, sizes, seed):
    from epstan_amd.engine import is_gauss
    rng = np.random.RandomState(seed)
    N = int(np.sum(sizes))
    X = rng.randn(N, D) * 1.5
    y = 0.4 + X.dot(rng.randn(D) * 0.5) + 0.8 * rng.randn(N) if is_gauss(model) else (rng.rand(N) < 0.6).astype(int)
    return X, y, np.concatenate(([0], np.cumsum(sizes)))


def entries(eng, tag, out, theta=None, chains=None, k0=0, count=None, seed=0):
    """All seven entries on the sites [k0, k0 + count); theta None: the draws the sampler left."""
    from epstan_amd import site_params
    from epstan_amd.engine import MODEL_IDS, is_gauss
    count = eng.K - k0 if count is None else count
    rng = np.random.RandomState(1000 + seed)
    names = site_params.names(MODEL_IDS[eng.model] % 5, is_gauss(eng.model))
    kw = dict(k0=k0, count=count, theta=theta)
    if eng.D <= 32:                                      # (the named entries' tests stop there)
        n, mean, m2 = eng.named_moments(names, **kw)
        ranks = np.unique([0, n // 4, n // 2, n - 1])
        stats = eng.named_order_stats(names, ranks, **kw)
        for b in range(count):
            for name in names:
                out['%s/mean/%d/%s' % (tag, b, name)] = mean[b][name]
                out['%s/m2/%d/%s' % (tag, b, name)] = m2[b][name]
                out['%s/order/%d/%s' % (tag, b, name)] = stats[b][name]
        hist, n_nan, n_all = eng.pooled_count_pass(['phi'], 56, None, 2, **kw)
        out[tag + '/count56'], out[tag + '/count56_nan'], out[tag + '/count_n'] = hist, n_nan, np.array(n_all)
        prefix = rng.randint(0, 2 ** 62, size=(eng.d, 2)).astype(np.uint64)
        hist, n_nan, _ = eng.pooled_count_pass(['phi'], 48, prefix, 2, **kw)
        out[tag + '/count48'], out[tag + '/count48_nan'] = hist, n_nan
    rows = 3
    Xn = rng.randn(rows * count, eng.D)
    group = None if eng.g_cnt is None else np.concatenate(
        [rng.randint(0, int(eng.g_cnt[k0 + b]), rows) for b in range(count)]).astype(np.int32)
    yn = rng.randn(rows * count) if is_gauss(eng.model) else (rng.rand(rows * count) < 0.5).astype(float)
    out[tag + '/predict'] = eng.predict(Xn, np.arange(count + 1) * rows, group, yn, **kw)
    out[tag + '/loo'] = eng.loo(**kw)
    out[tag + '/diag'] = eng.draw_diagnostics(chains=chains, **kw)
    n, s, sc = eng.pooled_moments(center=rng.randn(eng.d), **kw)
    out[tag + '/pooled_sum'], out[tag + '/pooled_scatter'], out[tag + '/pooled_n'] = s, sc, np.array(n)
    out[tag + '/pooled_sum_only'] = eng.pooled_moments(want_scatter=False, **kw)[1]


def later_entries(eng, tag, out, theta, new_rows, seed=0):
    """The entries over draws that came after those of `entries`, on all sites with injected draws of 4 chains:
    replicated_checks with the per-draw sums, site_evidence with its terms (120 draws of its own: the fit set needs 2 P),
    predict_order_stats of f and, Gaussian family, of the replicates (new_rows: new rows per site), draw_rank_diagnostics."""
    from epstan_amd.engine import is_gauss
    rng = np.random.RandomState(2000 + seed)
    S = theta.shape[1]
    groups, sites, draws = eng.replicated_checks(seed=5, row0=7, theta=theta, with_draws=True)
    out[tag + '/ppc_groups'], out[tag + '/ppc_sites'], out[tag + '/ppc_draws'] = groups, sites, draws
    if eng.D <= 32:                                      # (the proposal's factor of more coordinates does not fit the LDS)
        for k in range(eng.K):
            assert eng.cavity_site(k, 5.0 * np.eye(eng.d), np.zeros(eng.d), np.eye(eng.d), np.zeros(eng.d))
        records, terms, _ = eng.site_evidence(seed=3, site0=2, theta=0.5 * rng.randn(eng.K, 120, eng.P) + 0.3, chains=4,
                                              with_terms=True)
        out[tag + '/evidence'] = records
        for b, site in enumerate(terms):
            for key, value in site.items():
                out['%s/evidence_terms/%d/%s' % (tag, b, key)] = np.asarray(value)
    row_lim = np.concatenate(([0], np.cumsum(new_rows)))
    Xn = rng.randn(int(row_lim[-1]), eng.D)
    group = None if eng.g_cnt is None else np.concatenate(
        [rng.randint(0, int(eng.g_cnt[k]), n) for k, n in enumerate(new_rows)]).astype(np.int32)
    ranks = np.unique([0, S // 4, S // 2, S - 1])
    for what in ('f', 'yrep') if is_gauss(eng.model) else ('f',):
        out['%s/predict_order_%s' % (tag, what)] = eng.predict_order_stats(Xn, row_lim, ranks, group, what=what, seed=13,
                                                                           theta=theta)
    out[tag + '/rank_diag'] = eng.draw_rank_diagnostics(theta=theta, chains=4)


def tile_edges(out):
    """The predictive entries at the edges of their row-tile walk (csrc/predict_tile.h): an empty site, a full tile of 16
    rows, one row past a tile, one past a workgroup's 64; both homes of the LOO tile; a new group's pool of several
    chunks with a partial last slab."""
    from epstan_amd.engine import HipEngine, is_gauss
    K, S = 5, 40
    for model, D in (('m1b_sg', 3), ('m4b_sg', 3), ('m5b_sg', 3), ('m4a_sg', 3), ('m4b_sg', 128)):
        tag = 'tile/%s-D%d' % (model, D)
        rng = np.random.RandomState(500 + D)
        X, y, k_lim = problem(model, D, [4] * K, 77)
        eng = HipEngine(model, X, y, k_lim)
        theta = 0.5 * rng.randn(K, S, eng.P) + 0.3

        def responses(n):
            return rng.randn(n) if is_gauss(model) else (rng.rand(n) < 0.5).astype(float)

        row_lim = np.concatenate(([0], np.cumsum([3, 0, 16, 17, 65])))
        Xn = rng.randn(int(row_lim[-1]), D)
        out[tag + '/predict'] = eng.predict(Xn, row_lim, None, None, theta=theta)
        out[tag + '/predict_y'] = eng.predict(Xn, row_lim, None, responses(len(Xn)), theta=theta)
        # four labels: 65 rows, 17, 1 and none; N = 5 x 40 x 3 = 600 members are chunks of 256, 256 and 88 (5.5 slabs)
        gidx = rng.permutation(np.repeat([0, 1, 3], [65, 17, 1])).astype(np.int32)
        labels = np.array([5, 11, 2, 40], dtype=np.int32)
        Xg, yg = rng.randn(len(gidx), D), responses(len(gidx))
        for R in (1, 3):
            for name, yy in (('', None), ('_y', yg)):
                rows, glpd, N = eng.predict_new_group(Xg, gidx, labels, yy, seed=9, t0=3, R=R, theta=theta)
                out['%s/newgroup%s-R%d' % (tag, name, R)] = rows
                out['%s/newgroup%s-R%d-glpd' % (tag, name, R)] = glpd
                out['%s/newgroup%s-R%d-N' % (tag, name, R)] = np.array(N)
        out[tag + '/latents'] = eng.newgroup_latents(9, 11, 3, 17, 3)
        later_entries(eng, tag, out, theta, [3, 0, 16, 17, 65], seed=D)
        eng.close()
    for model in ('m4b_sg', 'm4a_sg'):
        X, y, k_lim = problem(model, 3, [7, 16, 17, 65], 78)
        eng = HipEngine(model, X, y, k_lim)
        theta = 0.5 * np.random.RandomState(226).randn(4, 226, eng.P) + 0.3
        for budget in (None, '0', '70000'):              # the LDS tile, the workspace tile, fewer tiles per work item
            if budget is not None:
                os.environ['EPX_LOO_LDS_BYTES'] = budget
            out['tile/%s/loo-lds-%s' % (model, budget)] = eng.loo(theta=theta)
        del os.environ['EPX_LOO_LDS_BYTES']
        eng.close()


def dump(path):
    from epstan_amd import _lib
    from epstan_amd.engine import HipEngine
    if _lib.device_count() < 1:
        raise SystemExit('draw_entries_dump.py needs a HIP device')
    out = {}
    tile_edges(out)
    for model in ('m1b_sg', 'm4b_sg', 'm4a_sg'):
        for D, chains, nkeep in SHAPES:
            K = 5
            X, y, k_lim = problem(model, D, [7] * K, 300 + D)
            eng = HipEngine(model, X, y, k_lim)
            theta = 0.5 * np.random.RandomState(7 * D + chains).randn(K, chains * nkeep, eng.P) + 0.3
            entries(eng, '%s-D%d' % (model, D), out, theta, chains, seed=D)
            entries(eng, '%s-D%d-sub' % (model, D), out, theta[1:4], chains, k0=1, count=3, seed=D)
            eng.close()
    for model in ('m4b', 'm1b', 'm4a'):
        X, y, k_lim = problem(model, 3, [int(np.sum(g)) for g in GROUPS], 23)
        g_cnt = np.array([len(g) for g in GROUPS], dtype=np.int32)
        g_lim = np.concatenate(([0], np.cumsum([n for g in GROUPS for n in g])))
        eng = HipEngine(model, X, y, k_lim, g_cnt=g_cnt, g_lim=g_lim)
        theta = 0.5 * np.random.RandomState(31).randn(3, 40, eng.P) + 0.3
        for k in range(3):                               # every site its own elements (the pool needs equal lengths)
            entries(eng, '%s-site%d' % (model, k), out, theta[k:k + 1], 4, k0=k, count=1, seed=k)
        out[model + '/loo-sub'] = eng.loo(k0=1, count=2, theta=theta[1:3])      # (a sub-range starts at its own first group)
        later_entries(eng, model + '-groups', out, theta, [3, 0, 17], seed=3)
        eng.close()
    # the sampler's own draws: a cavity of precision 4 I around 0 on every site, one short run
    K, D = 3, 3
    X, y, k_lim = problem('m4b_sg', D, [40] * K, 41)
    eng = HipEngine('m4b_sg', X, y, k_lim)
    for k in range(K):
        assert eng.cavity_site(k, 5.0 * np.eye(eng.d), np.zeros(eng.d), np.eye(eng.d), np.zeros(eng.d))
    eng.sample_batch(np.arange(11, 11 + K, dtype=np.int64), HipEngine.sampler_opts(chains=4, iter=80, init='random'))
    entries(eng, 'sampled', out, seed=1)
    entries(eng, 'sampled-sub', out, k0=1, count=2, seed=2)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print('%d arrays, %d numbers -> %s (%s)' % (len(out), sum(np.size(v) for v in out.values()), path, _lib.LIB_PATH))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), 'the two files hold different arrays'
    bad = [k for k in a.files if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    n_nan = sum(int(np.isnan(a[k]).sum()) for k in a.files if a[k].dtype.kind == 'f')
    print('%d arrays, %d numbers (%d NaN): %s' % (len(a.files), sum(a[k].size for k in a.files), n_nan,
                                                   'BIT-EQUAL' if not bad else 'DIFFERENT: %s' % bad[:10]))
    return 1 if bad else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--compare', nargs=2, default=None)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    dump(a.out or os.path.join(ROOT, 'results', 'draw_entries.npz'))
