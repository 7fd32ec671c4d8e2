"""`diagnostics.rank_normalize_host`, `diagnostics.rank_diagnostics_host` and `Master.diagnostics(rank=True)` on the CPU:
the NumPy statement of the rank-normalised split-Rhat, bulk-ESS and tail-ESS (include/epx.h, enum epx_rank_diag) against
facts that do not come from it -- SciPy's ranks, invariance under monotone maps, chains whose defect is known -- its NaN
rules, and `Master.diagnostics`' bookkeeping with the oracle standing in for the device engine."""

import numpy as np
import pytest
import scipy.special
import scipy.stats

from epstan_amd import diagnostics as dg
from epstan_amd.diagnostics import (DG_RHAT, RD_COUNT, RD_ESS_BULK, RD_ESS_TAIL, RD_RHAT, RD_RHAT_BULK, RD_RHAT_FOLD,
                                    diagnostics_host, rank_diagnostics_host, rank_normalize_host)

import test_predict_host as tph

CHAINS, NKEEP = 4, 200
N = CHAINS * NKEEP


# ------------------------------------------------------------------ ranks
def test_ranks_are_scipys_average_ranks():
    rng = np.random.RandomState(0)
    x = np.stack([rng.randn(257), np.round(2 * rng.randn(257)) / 2, rng.randint(0, 3, 257).astype(float)])
    rank, z = rank_normalize_host(x)
    for i in range(3):
        np.testing.assert_array_equal(rank[i], scipy.stats.rankdata(x[i], method='average'))
    np.testing.assert_array_equal(z, scipy.special.ndtri((rank - 0.375) / (257 + 0.25)))
    assert len(np.unique(x[1])) < 20 and np.all(np.diff(np.sort(z[0])) > 0)
    # folded: the ranks of |x - median|
    rank, _ = rank_normalize_host(x[0], fold=True)
    np.testing.assert_array_equal(rank, scipy.stats.rankdata(np.abs(x[0] - np.median(x[0])), method='average'))


def test_signed_zeros_tie_and_a_constant_series_has_the_middle_rank():
    rank, z = rank_normalize_host(np.array([0.0, -1.0, -0.0, 2.0, 0.0]))
    np.testing.assert_array_equal(rank, [3.0, 1.0, 3.0, 5.0, 3.0])
    assert z[0] == z[2] == z[4] == 0.0 and z[1] == -z[3]
    for n in (1, 2, 7, 800):
        rank, z = rank_normalize_host(np.full(n, -3.25))
        np.testing.assert_array_equal(rank, np.full(n, (n + 1) / 2.0))
        np.testing.assert_allclose(z, 0.0, atol=1e-15)
    rank, z = rank_normalize_host(np.array([[1.0, np.inf, 2.0], [1.0, 3.0, 2.0]]))
    assert np.all(np.isnan(rank[0])) and np.all(np.isnan(z[0])) and np.array_equal(rank[1], [1.0, 3.0, 2.0])


# ------------------------------------------------------------------ invariance under monotone maps
def test_monotone_maps_leave_every_field_bit_identical():
    """x, exp(x) and x ** 3 have the same ranks and the same indicators x <= q (an increasing map commutes with the
    order statistics up to the interpolation between two neighbours, which no draw lies between): the bulk and tail
    fields agree bit for bit.  The folded field is NOT invariant under these maps -- zeta = |x - med| orders the draws
    by their DISTANCE from the median, which exp and the cube change: on these draws RHAT_FOLD of coordinate 0 is
    0.99650 for x, 0.99698 for exp(x) and 0.99622 for x ** 3 -- so it is compared under the increasing maps that keep
    that order and are exact in floating point, the scalings by a power of two, where all five fields agree bit for
    bit."""
    x = np.random.RandomState(3).randn(N, 6)
    ref = rank_diagnostics_host(x, CHAINS)
    assert np.all(np.isfinite(ref))
    for f in (np.exp, lambda v: v ** 3):
        got = rank_diagnostics_host(f(x), CHAINS)
        assert np.all(np.isfinite(got))
        for col in (RD_RHAT_BULK, RD_ESS_BULK, RD_ESS_TAIL):
            assert got[:, col].tobytes() == ref[:, col].tobytes()
        assert np.max(np.abs(got[:, RD_RHAT_FOLD] - ref[:, RD_RHAT_FOLD])) < 0.01       # (another statistic, not far)
    for scale in (4.0, 0.25):
        assert rank_diagnostics_host(scale * x, CHAINS).tobytes() == ref.tobytes()


# ------------------------------------------------------------------ known answers at 4 x 200
def test_iid_normal_draws_have_about_n_effective_draws():
    rec = rank_diagnostics_host(np.random.RandomState(0).randn(N, 1), CHAINS)[0]
    print('iid normal: %s' % rec)
    assert 0.7 * N <= rec[RD_ESS_BULK] <= 1.3 * N and 0.7 * N <= rec[RD_ESS_TAIL] <= 1.3 * N
    assert rec[RD_RHAT] < 1.01 and rec[RD_RHAT] == max(rec[RD_RHAT_BULK], rec[RD_RHAT_FOLD])


def test_a_chain_three_times_as_wide_is_seen_by_the_folded_rhat_only():
    x = np.random.RandomState(0).randn(CHAINS, NKEEP, 1)
    x[3] *= 3.0
    x = x.reshape(N, 1)
    classic = diagnostics_host(x, CHAINS)[0, DG_RHAT]
    rec = rank_diagnostics_host(x, CHAINS)[0]
    print('one wide chain: classic %.4f, rank-normalised %s' % (classic, rec))
    assert classic < 1.01 and rec[RD_RHAT_FOLD] > 1.05 and rec[RD_RHAT] == rec[RD_RHAT_FOLD]


def test_a_shifted_chain_is_seen_by_the_bulk_rhat():
    x = np.random.RandomState(0).randn(CHAINS, NKEEP, 1)
    x[3] += 1.0
    rec = rank_diagnostics_host(x.reshape(N, 1), CHAINS)[0]
    print('one shifted chain: %s' % rec)
    assert rec[RD_RHAT_BULK] > 1.05


def test_cauchy_draws_have_finite_fields():
    x = np.random.RandomState(0).standard_cauchy((N, 3))
    assert np.abs(x).max() > 100.0
    rec = rank_diagnostics_host(x, CHAINS)
    assert np.all(np.isfinite(rec)) and np.all(rec[:, [RD_ESS_BULK, RD_ESS_TAIL]] > 0)


# ------------------------------------------------------------------ NaN rules
def test_nan_rules():
    x = np.random.RandomState(5).randn(N, 6)
    ref = rank_diagnostics_host(x, CHAINS)
    bad = x.copy()
    bad[17, 1] = np.nan
    bad[300, 2] = np.inf
    bad[:, 3] = 2.5                                          # a coordinate that never moved
    got = rank_diagnostics_host(bad, CHAINS)
    assert np.all(np.isnan(got[1:4])) and got[[0, 4, 5]].tobytes() == ref[[0, 4, 5]].tobytes()
    for chains, nkeep in ((4, 3), (4, 2), (1, 1), (2, 3)):   # nkeep < 4
        assert np.all(np.isnan(rank_diagnostics_host(x[:chains * nkeep], chains)))
    rec = rank_diagnostics_host(x[:4], 1)                    # (chains, nkeep) = (1, 4): M = 2, h = 2
    assert rec.shape == (6, RD_COUNT) and np.all(np.isfinite(rec))
    # a folded series that is constant (x symmetric about its median in two values): RHAT_FOLD and RHAT alone are NaN
    two = np.tile([-1.0, 1.0, 1.0, -1.0, 1.0, -1.0], 8)[:, None]
    rec = rank_diagnostics_host(two, 4)[0]
    assert np.isnan(rec[RD_RHAT]) and np.isnan(rec[RD_RHAT_FOLD]) and np.isfinite(rec[RD_RHAT_BULK])


# ------------------------------------------------------------------ Master.diagnostics(rank=True) on the oracle engine
RANK_KEYS = {'rhat_rank', 'rhat_bulk', 'rhat_folded', 'ess_bulk', 'ess_tail', 'site_max_rhat_rank', 'site_min_ess_rank'}
KEYS = {'mean', 'var', 'rhat', 'ess', 'ess_sq', 'mcse', 'n', 'site_max_rhat', 'site_min_ess', 'worst'}


def _check(M, chains=4):
    eng = M.engine
    assert not hasattr(eng, 'draw_rank_diagnostics')
    plain, res = M.diagnostics(), M.diagnostics(rank=True)
    assert set(plain) == KEYS and set(res) == KEYS | RANK_KEYS
    for key in KEYS - {'worst'}:
        np.testing.assert_array_equal(res[key], plain[key])
    assert res['worst'] == plain['worst']
    pg = (eng.P - eng.d) // int(M._site_ng[M.k_lo:M.k_hi].max())
    site_P = eng.d + M._site_ng * pg
    Pmax = int(site_P.max())
    rec = np.full((M.K, Pmax, RD_COUNT), np.nan)
    for k in range(M.K):
        theta = np.ascontiguousarray(eng.get_draws(k, all_params=True))[:, :site_P[k]]
        rec[k, :site_P[k]] = rank_diagnostics_host(theta, chains)
        assert np.all(np.isfinite(rec[k, :site_P[k], RD_RHAT_BULK])) and np.all(rec[k, :site_P[k], RD_ESS_BULK] > 0)
    for i, name in enumerate(dg.RD_NAMES):
        assert res[name].shape == (M.K, Pmax)
        np.testing.assert_array_equal(res[name], rec[:, :, i])
    np.testing.assert_array_equal(res['site_max_rhat_rank'], np.nanmax(rec[:, :, RD_RHAT], axis=1))
    np.testing.assert_array_equal(res['site_min_ess_rank'],
                                  np.nanmin(np.fmin(rec[:, :, RD_ESS_BULK], rec[:, :, RD_ESS_TAIL]), axis=1))
    return res, site_P


def test_master_rank_diagnostics_single_group():
    M, data = tph._sg_master()
    with pytest.raises(RuntimeError, match='at least one iteration'):
        M.diagnostics(rank=True)
    assert M.run(1, verbose=False, calc_moments=False, seed=2) == M.INFO_OK
    res, site_P = _check(M)
    assert np.all(np.isfinite(res['rhat_bulk'])) and not np.any(res['rhat_rank'] < res['rhat_bulk'])


def test_master_rank_diagnostics_with_several_groups_per_site():
    M, data, Nk, j_ind = tph._groups_master()                # 7 groups on 3 sites: 3 + 2 + 2
    M.run(1, verbose=False, seed=3)
    res, site_P = _check(M)
    assert len(set(site_P)) > 1
    for k in range(3):                                       # NaN exactly behind the site's own coordinates
        assert np.all(np.isfinite(res['ess_bulk'][k, :site_P[k]]))
        for name in dg.RD_NAMES:
            assert np.all(np.isnan(res[name][k, site_P[k]:]))


def test_summarise_skips_nan_and_keeps_an_all_nan_site_nan():
    rec = np.full((2, 3, 6), np.nan)
    rank = np.full((2, 3, RD_COUNT), np.nan)
    rank[0, :2] = [[1.02, 1.02, 1.01, 500.0, 300.0], [1.30, 1.01, 1.30, 90.0, 120.0]]
    res = dg.summarise(rec, [80, 80], rank)
    np.testing.assert_array_equal(res['site_max_rhat_rank'], [1.30, np.nan])
    np.testing.assert_array_equal(res['site_min_ess_rank'], [90.0, np.nan])
    assert set(dg.summarise(rec, [80, 80])) == KEYS
