"""k_predict_order / epx_predict_order_stats / Master.predict_quantiles on the device: order statistics across the draws of
new rows' linear predictor or replicated response, against predict_quantiles.predict_order_stats_host (NumPy) on the same
draws.  Need a real MI355X.

Tolerances (derived, not tuned).  An order statistic is 1-Lipschitz in the sup norm over the draws: if every value of a
row moves by at most e, every order statistic of the row moves by at most e.  Hence, per row i,
  EPX_PO_F     |got_(r) - host_(r)| <= max_s (1e-12 max(1, A_i) + 1e-9 |f_is|), test_gpu_predict.py's bound on f (A_i its
               `_scale`, 1e-9 its RTOL);
  EPX_PO_YREP  that bound on f, plus test_gpu_ppc.py's rule for what the replicate adds (the device's exp, log, sqrt and
               sincos): the host statement is evaluated in float64 and in np.longdouble and the device may differ from the
               float64 host by 100 x their largest difference over the case, floored at 1e-12 relative.
The sort itself is exact: sorted keys have one result, so everything about order, ties, multiplicities, the item size R
and the grid is compared bit for bit.  `Master.predict_quantiles`: the interpolation x_(i) + g (x_(i+1) - x_(i)), g in
[0, 1], is a convex combination, so a quantile carries the row's bound (plus the rounding of the form, 4 x 2^-53
relative); through the sigmoid, whose slope is at most 1/4, a quarter of it.
Measured on an MI355X (largest error / bound over all cases; test_zz_report prints every case): 7.3e-6 for EPX_PO_F, 7.9e-6
for EPX_PO_YREP, absolute errors up to 7.1e-14."""

import ctypes
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from epstan_amd import _lib, fit, predict_quantiles as pq, quantiles, site_params   # noqa: E402
from epstan_amd.draw_queries import INTERVALS, HostDraws                              # noqa: E402
from epstan_amd.engine import HipEngine, MODEL_IDS, is_gauss                          # noqa: E402
from test_gpu_parity import _site_problem, _group_problem                             # noqa: E402
from test_gpu_predict import _scale, RTOL                                             # noqa: E402

LD = np.longdouble
EPS = 2.0 ** -53
PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)
WORST = {}


def _spec(model):
    return MODEL_IDS[model] % 5, is_gauss(model)


def _ranks(S):
    """All ranks while they fit one call, else those of the default probabilities."""
    return np.arange(S, dtype=np.int64) if S <= 32 else quantiles.rank_plan(S, PROBS)[0]


def _row_bounds(model, D, site_ng, thetas, Xn, lim, group, what, seed, row_id):
    """(n) the error allowed in every order statistic of every row (module docstring)."""
    mid, gauss = _spec(model)
    n = Xn.shape[0]
    bound = np.zeros(n)
    ids = np.arange(n, dtype=np.int64) if row_id is None else np.asarray(row_id, dtype=np.int64)
    wide = []
    for k, ng in enumerate(site_ng):
        lo, hi = int(lim[k]), int(lim[k + 1])
        if hi == lo:
            continue
        grp = np.zeros(hi - lo, dtype=np.int64) if group is None else np.asarray(group[lo:hi], dtype=np.int64)
        f = site_params.linear_predictor(mid, D, ng, gauss, thetas[k], Xn[lo:hi], grp)
        A = np.maximum(1.0, _scale(model, D, ng, thetas[k], Xn[lo:hi], grp))
        with np.errstate(invalid='ignore'):
            bound[lo:hi] = 1e-12 * A + RTOL * np.abs(f).max(axis=0)
        if what == 'yrep':
            v = pq.site_values(mid, D, ng, gauss, thetas[k], Xn[lo:hi], grp, what, seed, ids[lo:hi])
            with np.errstate(all='ignore'):
                vw = pq.site_values(mid, D, ng, gauss, thetas[k], Xn[lo:hi], grp, what, seed, ids[lo:hi], dtype=LD)
            wide.append((lo, hi, np.abs(v).max(axis=0), float(np.abs((v - vw).astype(np.float64)).max())))
    if wide:
        ref = max(w[3] for w in wide)                       # over the case
        for lo, hi, vmax, _ in wide:
            bound[lo:hi] += np.maximum(100.0 * ref, 1e-12 * vmax)
    return bound


def _check(model, D, site_ng, thetas, Xn, lim, group, ranks, got, label, what='f', seed=0, row_id=None):
    """`got` (n, len(ranks)) against the host statement on the same draws; records the largest error / bound."""
    mid, gauss = _spec(model)
    host = pq.predict_order_stats_host(mid, D, site_ng, gauss, thetas, Xn, lim, ranks, group, what, seed, row_id)
    assert got.shape == host.shape == (Xn.shape[0], len(ranks)), label
    assert np.all(np.isfinite(host)) and np.all(np.isfinite(got)), label
    assert np.all(np.diff(got, axis=1) >= 0), label + ': a row is non-decreasing, exactly'
    bound = _row_bounds(model, D, site_ng, thetas, Xn, lim, group, what, seed, row_id)
    err = np.abs(got - host)
    ratio = float((err / bound[:, None]).max()) if err.size else 0.0
    print('%s: largest error %.3e, largest error / bound %.3e' % (label, err.max() if err.size else 0.0, ratio))
    assert np.all(err <= bound[:, None]), label
    WORST[label] = max(WORST.get(label, 0.0), ratio)
    return host


# ------------------------------------------------------------------ (a) values against the host, every model family
ROWS = np.array([3, 0, 16, 17, 33])      # an empty site, a full tile, one row past a tile, three tiles


@pytest.mark.parametrize('model', ['m1b_sg', 'm2b_sg', 'm3b_sg', 'm4b_sg', 'm5b_sg', 'm1a_sg', 'm4a_sg'])
@pytest.mark.parametrize('D,S', [(1, 1), (1, 2), (3, 15), (3, 16), (3, 17), (21, 100), (32, 400), (128, 33)])
def test_injected_draws_match_the_host_order_statistics(model, D, S):
    K = 5
    X, y, k_lim, _, _, d, P = _site_problem(model, D, 7, 300 + D, K=K)
    eng = HipEngine(model, X, y, k_lim)
    rng = np.random.RandomState(7 + D + S)
    theta = 0.5 * rng.randn(K, S, P) + 0.3
    lim = np.concatenate(([0], np.cumsum(ROWS)))
    n = int(lim[-1])
    Xn = 1.5 * rng.randn(n, D)
    ranks = _ranks(S)
    got, ns = eng.predict_order_stats(Xn, lim, ranks, theta=theta, with_n=True)
    assert ns == S
    label = '%s D=%d S=%d' % (model, D, S)
    _check(model, D, [1] * K, list(theta), Xn, lim, None, ranks, got, label + ' f')
    sub = eng.predict_order_stats(Xn[lim[1]:lim[4]], lim[1:5] - lim[1], ranks, k0=1, count=3, theta=theta[1:4])
    assert sub.tobytes() == got[lim[1]:lim[4]].tobytes()                # a sub-range: the same rows, the same bits
    if is_gauss(model):
        ids = rng.permutation(2 ** 20)[:n].astype(np.int64) * 4093      # stream indices up to 2^32, odd and even
        assert ids.max() < 2 ** 32 and ids.max() >= 2 ** 31
        rep = eng.predict_order_stats(Xn, lim, ranks, what='yrep', seed=1000 + S, row_id=ids, theta=theta)
        _check(model, D, [1] * K, list(theta), Xn, lim, None, ranks, rep, label + ' yrep', 'yrep', 1000 + S, ids)
        assert np.all(rep != got)
    else:
        with pytest.raises(_lib.EpxError, match='Gaussian family only'):
            eng.predict_order_stats(Xn, lim, ranks, what='yrep', theta=theta)
    eng.close()


# ------------------------------------------------------------------ (b) the sort, exactly
def _one_site(S, D=3, n=21, seed=3, model='m1b_sg'):
    X, y, k_lim, _, _, d, P = _site_problem(model, D, 7, 5, K=1)
    eng = HipEngine(model, X, y, k_lim)
    rng = np.random.RandomState(seed)
    return eng, 0.5 * rng.randn(1, S, P) + 0.3, 1.5 * rng.randn(n, D), np.array([0, n]), rng


def test_permuted_draws_give_the_same_bytes():
    """The order statistics are a function of the SET of a site's draws: a column's product does not depend on its slot of
    the slab, and sorted keys have one result."""
    S = 100
    eng, theta, Xn, lim, rng = _one_site(S)
    ranks = np.unique(np.concatenate(([0, S - 1], np.linspace(0, S - 1, 30).astype(np.int64))))
    base = eng.predict_order_stats(Xn, lim, ranks, theta=theta)
    f = site_params.linear_predictor(0, 3, 1, False, theta[0], Xn, None)
    for name, order in (('reversed', np.arange(S)[::-1]), ('sorted by row 4', np.argsort(f[:, 4])),
                        ('random', rng.permutation(S))):
        got = eng.predict_order_stats(Xn, lim, ranks, theta=np.ascontiguousarray(theta[:, order]))
        assert got.tobytes() == base.tobytes(), name
    eng.close()


def test_ties_multiplicities_and_the_extreme_ranks():
    S = 21
    eng, theta, Xn, lim, rng = _one_site(S)
    every = np.arange(S, dtype=np.int64)
    a, b = theta[0, 0].copy(), theta[0, 1].copy()
    same = np.ascontiguousarray(np.broadcast_to(a, theta.shape))
    fa = eng.predict_order_stats(Xn, lim, every, theta=same)
    assert np.all(fa.view(np.uint64) == fa[:, :1].view(np.uint64))      # one value at every rank, bit for bit
    fb = eng.predict_order_stats(Xn, lim, every, theta=np.ascontiguousarray(np.broadcast_to(b, theta.shape)))
    np.testing.assert_allclose(fa[:, 0], site_params.linear_predictor(0, 3, 1, False, a[None, :], Xn, None)[0], rtol=1e-9)
    assert np.all(fa[:, 0] != fb[:, 0])
    mixed = theta.copy()
    mixed[0, 0::2], mixed[0, 1::2] = a, b                               # 11 times a, 10 times b, interleaved
    got = eng.predict_order_stats(Xn, lim, every, theta=mixed)
    exp = np.sort(np.concatenate((np.repeat(fa[:, :1], 11, axis=1), np.repeat(fb[:, :1], 10, axis=1)), axis=1), axis=1)
    assert got.tobytes() == exp.tobytes()
    S = 32
    theta = 0.5 * rng.randn(1, S, theta.shape[2]) + 0.3
    full = eng.predict_order_stats(Xn, lim, np.arange(S), theta=theta)
    ends = eng.predict_order_stats(Xn, lim, [0, S - 1], theta=theta)
    assert ends.tobytes() == np.ascontiguousarray(full[:, [0, S - 1]]).tobytes()
    assert np.all(ends[:, 0] == full.min(axis=1)) and np.all(ends[:, 1] == full.max(axis=1))
    eng.close()


# ------------------------------------------------------------------ (c) R < 16 and the draw limit
def test_smaller_items_give_the_same_bytes(monkeypatch):
    """EPX_PO_LDS_BYTES lowers the keys' budget: at S = 100 (N = 128) an item of R rows needs R x 1024 bytes."""
    D, S, K = 3, 100, 3
    X, y, k_lim, _, _, d, P = _site_problem('m4a_sg', D, 7, 5, K=K)
    eng = HipEngine('m4a_sg', X, y, k_lim)
    rng = np.random.RandomState(1)
    theta = 0.5 * rng.randn(K, S, P) + 0.3
    lim = np.array([0, 33, 33, 50])
    Xn = 1.5 * rng.randn(50, D)
    ranks = _ranks(S)
    monkeypatch.delenv('EPX_PO_LDS_BYTES', raising=False)
    base = dict((what, eng.predict_order_stats(Xn, lim, ranks, what=what, seed=4, theta=theta)) for what in ('f', 'yrep'))
    _check('m4a_sg', D, [1] * K, list(theta), Xn, lim, None, ranks, base['f'], 'R=16 S=100 f')
    _check('m4a_sg', D, [1] * K, list(theta), Xn, lim, None, ranks, base['yrep'], 'R=16 S=100 yrep', 'yrep', 4)
    for R in (8, 4, 2, 1):
        monkeypatch.setenv('EPX_PO_LDS_BYTES', str(R * 128 * 8))
        for what in ('f', 'yrep'):
            got = eng.predict_order_stats(Xn, lim, ranks, what=what, seed=4, theta=theta)
            assert got.tobytes() == base[what].tobytes(), (R, what)
    for S2 in (64, 65):                                                 # a power of two and one beyond, R = 16 and R = 2
        th = 0.5 * rng.randn(K, S2, P) + 0.3
        r2 = _ranks(S2)
        monkeypatch.delenv('EPX_PO_LDS_BYTES')
        got = eng.predict_order_stats(Xn, lim, r2, theta=th)
        _check('m4a_sg', D, [1] * K, list(th), Xn, lim, None, r2, got, 'S=%d f' % S2)
        monkeypatch.setenv('EPX_PO_LDS_BYTES', str(2 * (64 if S2 == 64 else 128) * 8))
        assert eng.predict_order_stats(Xn, lim, r2, theta=th).tobytes() == got.tobytes(), S2
    eng.close()


def test_the_draw_limit(monkeypatch):
    D, K = 3, 2
    X, y, k_lim, _, _, d, P = _site_problem('m1b_sg', D, 7, 5, K=K)
    eng = HipEngine('m1b_sg', X, y, k_lim)
    rng = np.random.RandomState(2)
    lim = np.array([0, 5, 22])
    Xn = 1.5 * rng.randn(22, D)
    monkeypatch.setenv('EPX_PO_LDS_BYTES', '1024')                      # 128 keys: the limit, at R = 1
    theta = 0.5 * rng.randn(K, 129, P) + 0.3
    at = np.ascontiguousarray(theta[:, :128])
    ranks = _ranks(128)
    got = eng.predict_order_stats(Xn, lim, ranks, theta=at)
    _check('m1b_sg', D, [1] * K, list(at), Xn, lim, None, ranks, got, 'S at the lowered limit')
    with pytest.raises(_lib.EpxError, match=r'S = 129 draws per site, at most 128 .*EPX_PO_LDS_BYTES = 1024'):
        eng.predict_order_stats(Xn, lim, ranks, theta=theta)              # (the refusal names the variable that lowered it)
    for junk in ('', 'lots', '12k', '-1'):                              # no whole non-negative number: ignored
        monkeypatch.setenv('EPX_PO_LDS_BYTES', junk)
        assert eng.predict_order_stats(Xn, lim, ranks, theta=theta).shape == (22, len(ranks))
    monkeypatch.delenv('EPX_PO_LDS_BYTES')
    # a raw call with S = 10^7 over a small buffer: refused before anything is read
    out = np.full((22, 2), 7.0)
    r01 = np.array([0, 1], dtype=np.int64)
    small = np.zeros((K, 4, P))
    rc = eng.lib.epx_predict_order_stats(eng.ctx, 0, K, lim.ctypes.data_as(_lib.c_int64_p), None, _lib.dptr(Xn), None, 0,
                                         ctypes.c_uint64(0), r01.ctypes.data_as(_lib.c_int64_p), 2, _lib.dptr(small),
                                         10 ** 7, _lib.dptr(out), None)
    text = eng.lib.epx_last_error().decode()
    m = re.search(r'S = 10000000 draws per site, at most (\d+)', text)
    assert rc != 0 and m and int(m.group(1)) == 16384, text             # 128 KiB of keys in the 160 KiB of LDS
    assert np.all(out == 7.0)
    eng.close()


# ------------------------------------------------------------------ (d) sites with several groups
@pytest.mark.parametrize('model', ['m4b', 'm1b'])
def test_multi_group_sites_own_coordinates_and_row_order(model):
    D, S, groups = 3, 30, [[9], [8, 7, 9], [10, 6]]
    K = len(groups)
    X, y, k_lim, g_cnt, g_lim, _, _, d = _group_problem(model, D, groups, 23)
    eng = HipEngine(model, X, y, k_lim, g_cnt=g_cnt, g_lim=g_lim)
    rng = np.random.RandomState(3)
    theta = np.full((K, S, eng.P), np.nan)                              # NaN behind every site's own coordinates
    for k in range(K):
        theta[k, :, :eng.site_P[k]] = 0.5 * rng.randn(S, eng.site_P[k]) + 0.3
    thetas = [theta[k, :, :eng.site_P[k]] for k in range(K)]
    # new rows in group order: 20 (more than a tile) in every site's first group, 3 in the others, none in the last of all
    per_group = [[20] + [3] * (len(g) - 1) for g in groups]
    per_group[-1][-1] = 0
    cnt = np.array([sum(p) for p in per_group])
    lim = np.concatenate(([0], np.cumsum(cnt)))
    group = np.concatenate([np.repeat(np.arange(len(p)), p) for p in per_group]).astype(np.int32)
    Xn = 1.2 * rng.randn(int(lim[-1]), D)
    ranks = _ranks(S)
    got = eng.predict_order_stats(Xn, lim, ranks, row_group=group, theta=theta)
    _check(model, D, [int(g) for g in g_cnt], thetas, Xn, lim, group, ranks, got, '%s groups in order' % model)
    mix = np.concatenate([lim[k] + rng.permutation(cnt[k]) for k in range(K)])      # the groups of a site mixed
    got2 = eng.predict_order_stats(Xn[mix], lim, ranks, row_group=group[mix], theta=theta)
    assert got2.tobytes() == got[mix].tobytes()                         # a row's result does not depend on its place
    eng.close()


# ------------------------------------------------------------------ (e) more work items than the grid holds
def test_a_workgroup_walks_its_items():
    """1100 work items on at most 512 workgroups (two on each of 256 compute units): a workgroup starts its next item with
    cleared flags and fresh pads -- the NaN planted in site 3 stays there."""
    K, D, S = 1100, 1, 17
    X, y, k_lim, _, _, d, P = _site_problem('m1b_sg', D, 2, 9, K=K)
    eng = HipEngine('m1b_sg', X, y, k_lim)
    rng = np.random.RandomState(4)
    theta = 0.5 * rng.randn(K, S, P) + 0.3
    lim = 2 * np.arange(K + 1)
    Xn = 1.5 * rng.randn(2 * K, D)
    ranks = _ranks(S)
    got = eng.predict_order_stats(Xn, lim, ranks, theta=theta)
    _check('m1b_sg', D, [1] * K, list(theta), Xn, lim, None, ranks, got, '1100 items')
    theta[3, 5, 0] = np.nan
    bad = eng.predict_order_stats(Xn, lim, ranks, theta=theta)
    hit = np.repeat(np.arange(K) == 3, 2)
    assert np.all(np.isnan(bad[hit])) and bad[~hit].tobytes() == got[~hit].tobytes()
    eng.close()


# ------------------------------------------------------------------ (f) the same bits whatever the call
def test_same_bits_whatever_the_call():
    D, S, K = 3, 33, 4
    X, y, k_lim, _, _, d, P = _site_problem('m4a_sg', D, 7, 5, K=K)
    eng = HipEngine('m4a_sg', X, y, k_lim)
    rng = np.random.RandomState(6)
    theta = 0.5 * rng.randn(K, S, P) + 0.3
    lim = np.array([0, 19, 20, 20, 41])
    n = 41
    Xn = 1.5 * rng.randn(n, D)
    ranks = _ranks(S)
    ids = (rng.permutation(1000)[:n] * 3 + 1000).astype(np.int64)      # (none of them a row's position)
    for what in ('f', 'yrep'):
        kw = dict(what=what, seed=8)
        one = eng.predict_order_stats(Xn, lim, ranks, row_id=ids, theta=theta, **kw)
        two = eng.predict_order_stats(Xn, lim, ranks, row_id=ids, theta=theta, **kw)
        assert one.tobytes() == two.tobytes()                           # twice
        head = eng.predict_order_stats(Xn[:19], lim[:2], ranks, row_id=ids[:19], k0=0, count=1, theta=theta[:1], **kw)
        tail = eng.predict_order_stats(Xn[19:], lim[1:] - 19, ranks, row_id=ids[19:], k0=1, count=K - 1, theta=theta[1:], **kw)
        assert one.tobytes() == np.concatenate((head, tail)).tobytes()  # [0, K) = [0, 1) and [1, K) side by side
        # the rows of every site in another order, each with its own stream index
        mix = np.concatenate([lim[k] + rng.permutation(lim[k + 1] - lim[k]) for k in range(K)])
        moved = eng.predict_order_stats(Xn[mix], lim, ranks, row_id=ids[mix], theta=theta, **kw)
        assert moved.tobytes() == one[mix].tobytes()
        other = eng.predict_order_stats(Xn, lim, ranks, row_id=ids, theta=theta, what=what, seed=9)
        if what == 'f':
            assert other.tobytes() == one.tobytes()                     # f does not see the seed, nor the indices
            assert eng.predict_order_stats(Xn, lim, ranks, theta=theta).tobytes() == one.tobytes()
        else:
            assert np.all(other != one)
            pos = eng.predict_order_stats(Xn, lim, ranks, theta=theta, **kw)          # row_id None: the position
            assert pos.tobytes() == eng.predict_order_stats(Xn, lim, ranks, row_id=np.arange(n), theta=theta, **kw).tobytes()
            assert np.all(pos != one)
    eng.close()


# ------------------------------------------------------------------ (g) NaN and inf
def test_nan_stays_in_its_group_and_inf_sorts_to_the_ends():
    D, S, groups = 3, 20, [[9], [8, 7, 9], [10, 6]]
    K = len(groups)
    X, y, k_lim, g_cnt, g_lim, _, _, d = _group_problem('m4b', D, groups, 23)
    eng = HipEngine('m4b', X, y, k_lim, g_cnt=g_cnt, g_lim=g_lim)
    rng = np.random.RandomState(5)
    theta = np.full((K, S, eng.P), np.nan)
    for k in range(K):
        theta[k, :, :eng.site_P[k]] = 0.5 * rng.randn(S, eng.site_P[k]) + 0.3
    cnt = np.array([4, 18, 6])
    lim = np.concatenate(([0], np.cumsum(cnt)))
    group = np.concatenate((np.zeros(4), np.arange(18) % 3, np.arange(6) % 2)).astype(np.int32)
    Xn = 1.2 * rng.randn(28, D)
    Xn[np.abs(Xn) < 1e-3] = 0.5
    ranks = _ranks(S)
    good = eng.predict_order_stats(Xn, lim, ranks, row_group=group, theta=theta)
    assert np.all(np.isfinite(good))
    dd = eng.d
    kept = theta[1, 13, dd + 1]
    theta[1, 13, dd + 1] = np.nan                                       # eta of group 1 of site 1, one draw
    got = eng.predict_order_stats(Xn, lim, ranks, row_group=group, theta=theta)
    hit = (np.arange(28) >= 4) & (np.arange(28) < 22) & (group == 1)
    assert hit.sum() == 6 and np.all(np.isnan(got[hit])) and got[~hit].tobytes() == good[~hit].tobytes()
    theta[1, 13, dd + 1] = kept
    eng.close()
    # +inf in one coefficient of one draw: +inf at the top rank of the rows with a positive covariate, -inf at rank 0 of
    # those with a negative one, and the ranks between are the other draws'
    X, y, k_lim, _, _, d, P = _site_problem('m1b_sg', D, 7, 5, K=1)
    eng = HipEngine('m1b_sg', X, y, k_lim)
    th = 0.5 * rng.randn(1, S, P) + 0.3
    Xr = Xn[:9]
    base = eng.predict_order_stats(Xr, [0, 9], ranks, theta=th)
    th[0, 7, 2] = np.inf                                                # phi = [log sigma_a, beta]: beta_1 of draw 7
    got = eng.predict_order_stats(Xr, [0, 9], ranks, theta=th)
    up = Xr[:, 1] > 0
    assert up.any() and (~up).any()
    assert np.all(got[up, -1] == np.inf) and np.all(got[~up, 0] == -np.inf)
    assert np.all(np.isfinite(got[up, :-1])) and np.all(np.isfinite(got[~up, 1:]))
    exp = pq.predict_order_stats_host(0, D, [1], False, [th[0]], Xr, [0, 9], ranks)
    inner = np.isfinite(exp)
    np.testing.assert_allclose(got[inner], exp[inner], rtol=1e-9, atol=1e-11)
    assert np.array_equal(np.isfinite(got), inner) and np.all(np.isfinite(base))
    eng.close()


# ------------------------------------------------------------------ (h) refusals
def _raw(eng, lim, Xn, ranks, theta, S, out, k0=0, count=None, what=0, row_id=None, n_ranks=None, group=None, nsamp=None):
    lim = np.ascontiguousarray(lim, dtype=np.int64)
    ranks = np.ascontiguousarray(ranks, dtype=np.int64)
    ids = None if row_id is None else np.ascontiguousarray(row_id, dtype=np.int64)
    grp = None if group is None else np.ascontiguousarray(group, dtype=np.int32)
    return eng.lib.epx_predict_order_stats(
        eng.ctx, k0, eng.K if count is None else count, lim.ctypes.data_as(_lib.c_int64_p),
        None if grp is None else grp.ctypes.data_as(_lib.c_int32_p), _lib.dptr(Xn),
        None if ids is None else ids.ctypes.data_as(_lib.c_int64_p), what, ctypes.c_uint64(0),
        ranks.ctypes.data_as(_lib.c_int64_p), len(ranks) if n_ranks is None else n_ranks, _lib.dptr(theta), S, _lib.dptr(out),
        None if nsamp is None else ctypes.byref(nsamp))


def test_refusals_launch_nothing():
    D, K, S = 2, 2, 8
    X, y, k_lim, _, _, d, P = _site_problem('m1b_sg', D, 3, 5, K=K)
    eng = HipEngine('m1b_sg', X, y, k_lim)
    theta = np.zeros((K, S, P))
    Xn, lim = np.ones((5, D)), np.array([0, 2, 5])
    out = np.full((5, 33), 7.0)

    def refused(match, **kw):
        args = dict(lim=lim, Xn=Xn, ranks=[0, 3], theta=theta, S=S, out=out)
        args.update(kw)
        assert _raw(eng, **args) != 0
        text = eng.lib.epx_last_error().decode()
        assert re.search(match, text), text

    assert _raw(eng, lim, Xn, [0, 3], theta, S, out) == 0 and np.all(out.ravel()[:10] == 0.0)      # the call that works
    out[:] = 7.0
    refused('between 1 and 32 ranks', ranks=[0], n_ranks=0)
    refused('between 1 and 32 ranks', ranks=np.arange(33), n_ranks=33)
    refused('ascending and distinct', ranks=[3, 0])
    refused('ascending and distinct', ranks=[2, 2])
    refused(r'rank 8 outside \[0, 8\)', ranks=[0, 8])
    refused(r'rank -1 outside', ranks=[-1, 2])
    refused('S = 0', S=0)
    refused('what = 2', what=2)
    refused('what = -1', what=-1)
    refused('Gaussian family only', what=pq.PO_YREP)
    refused(r'row 3: row_id = 4294967296 outside \[0,2\^32\)', row_id=[0, 1, 2, 2 ** 32, 4])
    refused(r'row 0: row_id = -1 outside', row_id=[-1, 1, 2, 3, 4])
    refused('site range', k0=1, count=2, lim=lim)
    refused('site range', k0=-1, count=1, lim=lim[:2])
    refused('site range', count=0, lim=lim[:1])
    refused('start at 0', lim=[1, 2, 5])
    refused('non-decreasing', lim=[0, 6, 5])
    ns = ctypes.c_int(-5)                                               # the last refusal of all leaves nsamp alone too
    refused('row 1: group 1 outside the 1 group', group=[0, 1, 0, 0, 0], nsamp=ns)
    assert ns.value == -5
    refused('no draws yet', theta=None, S=0)                            # the draws of a sampling call there has not been
    with pytest.raises(_lib.EpxError, match='no draws yet'):
        eng.predict_order_stats(Xn, lim, [0, 3])
    assert np.all(out == 7.0)                                           # nothing was written
    ns = ctypes.c_int()                                                 # n = 0: nothing launched, nothing written
    zero = np.zeros(3, dtype=np.int64)
    r03 = np.array([0, 3], dtype=np.int64)
    _lib.check(eng.lib.epx_predict_order_stats(eng.ctx, 0, K, zero.ctypes.data_as(_lib.c_int64_p), None, None, None, 0,
                                               ctypes.c_uint64(0), r03.ctypes.data_as(_lib.c_int64_p), 2, _lib.dptr(theta), S,
                                               _lib.dptr(out), ctypes.byref(ns)))
    assert ns.value == S and np.all(out == 7.0)
    eng.close()
    D = 129                                                             # EPX_PR_DMAX = 128
    rng = np.random.RandomState(2)
    eng = HipEngine('m1b_sg', rng.randn(2, D), np.array([0, 1]), np.array([0, 2]))
    with pytest.raises(_lib.EpxError, match='D = 129 columns, at most 128'):
        eng.predict_order_stats(np.ones((1, D)), [0, 1], [0], theta=np.zeros((1, 4, eng.P)))
    out = np.full((1, 2), 7.0)
    assert _raw(eng, [0, 1], np.ones((1, D)), [0], np.zeros((1, 4, eng.P)), 4, out) != 0
    assert b'D = 129 columns, at most 128' in eng.lib.epx_last_error() and np.all(out == 7.0)
    eng.close()


# ------------------------------------------------------------------ (i) Master.predict_quantiles on the device
class _Spy(object):
    """Counts the calls of INTERVALS that reach `target`."""

    def __init__(self, target):
        self.target, self.calls = target, []

    def __getattr__(self, name):
        if name not in INTERVALS:
            raise AttributeError(name)
        self.calls.append(name)
        return getattr(self.target, name)


@pytest.mark.parametrize('name,J,K', [('m4b', 4, 2), ('m4b', 3, 3), ('m4a', 4, 2)])
def test_master_predict_quantiles_on_the_device(name, J, K):
    """The device route `Master` takes as built against the host route forced over the same `HipEngine`: both read the
    same device draws (the pattern of test_gpu_ppc.py)."""
    D = 2
    conf = fit.configurations(J=J, D=D, K=K, npg=30, siter=40, chains=4, run_ep=True, damp=0.4)
    M = fit.main(name, conf, ret_master=True)
    assert isinstance(M.engine, HipEngine) and isinstance(M._queries.host, HostDraws)
    multi = not M.model_name.endswith('_sg')
    assert multi == (K < J)
    j_ind = np.asarray(M.A_n['j_ind']) if multi else None
    with pytest.raises(RuntimeError, match='before at least one iteration'):
        M.predict_quantiles(M.X, site_sizes=M.Nk, j_ind=j_ind)
    assert M.run(1, verbose=False, calc_moments=False, seed=5) == 0
    gauss = is_gauss(M.model_name)
    S = M.engine.num_draws()
    ranks, plan = quantiles.rank_plan(S, PROBS)
    thetas = [np.ascontiguousarray(M.engine.get_draws(k, all_params=True))[:, :M.engine.site_P[k] if multi else None]
              for k in range(K)]
    group = j_ind - 1 if multi else None
    site_ng = [int(g) for g in M._site_ng]
    for scale in ('linear', 'mean') + (('response',) if gauss else ()):
        kw = dict(site_sizes=M.Nk, j_ind=j_ind, scale=scale, seed=3)
        dev = M.predict_quantiles(M.X, **kw)
        resolver = M._queries
        spy = M._queries = _Spy(resolver.host)
        try:
            host = M.predict_quantiles(M.X, **kw)
        finally:
            M._queries = resolver
        assert spy.calls == ['predict_order_stats']
        assert dev['n'] == host['n'] == S and dev['scale'] == scale and dev['quantiles'].shape == (5, M.N)
        what = 'yrep' if scale == 'response' else 'f'
        ids = np.arange(M.N, dtype=np.int64)
        raw = M.engine.predict_order_stats(M.X, M.k_lim, ranks, group, what=what, seed=3, row_id=ids)
        through = scale == 'mean' and not gauss
        again = pq.quantiles_of(raw, ranks, plan, through)              # the dict is the interpolation of the engine's records
        assert dev['quantiles'].tobytes() == again.tobytes()
        label = 'Master %s J=%d K=%d %s' % (name, J, K, scale)
        _check(M.model_name, D, site_ng, thetas, M.X, M.k_lim, group, ranks, raw, label, what, 3, ids)
        bound = _row_bounds(M.model_name, D, site_ng, thetas, M.X, M.k_lim, group, what, 3, ids)
        bound = (0.25 if through else 1.0) * bound[None, :] + 4 * EPS * np.abs(host['quantiles'])
        err = np.abs(dev['quantiles'] - host['quantiles'])
        print('%s quantiles: largest error / bound %.3e' % (label, (err / bound).max()))
        assert np.all(err <= bound), label
        if through:
            assert np.all((dev['quantiles'] > 0) & (dev['quantiles'] < 1))
    if not gauss:
        with pytest.raises(ValueError, match='Bernoulli'):
            M.predict_quantiles(M.X, site_sizes=M.Nk, j_ind=j_ind, scale='response')
    shuffle = np.random.RandomState(0).permutation(M.N)                 # any order of the rows, by site index
    one = M.predict_quantiles(M.X, site_sizes=M.Nk, j_ind=j_ind)
    two = M.predict_quantiles(M.X[shuffle], site_ind=np.asarray(M.k_ind)[shuffle], j_ind=j_ind[shuffle] if multi else None)
    assert two['quantiles'].tobytes() == np.ascontiguousarray(one['quantiles'][:, shuffle]).tobytes()


def test_zz_report():
    """The largest error / bound of every case above."""
    for what, worst in sorted(WORST.items()):
        print('%-44s largest error / bound %.3e' % (what, worst))
    for kind in (' f', ' yrep'):
        over = [w for what, w in WORST.items() if what.endswith(kind)]
        if over:
            print('over all cases,%s: %.3e' % (kind, max(over)))
    if WORST:
        print('over all cases: %.3e' % max(WORST.values()))
