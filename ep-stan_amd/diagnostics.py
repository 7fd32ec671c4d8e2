"""Per-coordinate sampler diagnostics of one site's draws in plain NumPy: split-Rhat, effective sample sizes and the
Monte-Carlo standard error of the tilted mean.  The definition is stated in include/epx.h (enum epx_diag); the device
kernel k_draw_diag (csrc/draw_diag.hip) computes the same next to the draws.  `diagnostics_host` is the expectation of
the kernel's tests and `Master.diagnostics`' route on an engine without `draw_diagnostics`.  `rank_diagnostics_host` is
the same for the rank-normalised split-Rhat, bulk-ESS and tail-ESS (enum epx_rank_diag; kernel k_rank_diag,
csrc/rank_diag.hip)."""

import numpy as np
from scipy.special import ndtri

from . import quantiles as _quantiles

# enum epx_diag (include/epx.h): the columns of a diagnostics record
DG_MEAN, DG_VAR, DG_RHAT, DG_ESS, DG_MCSE, DG_ESS_SQ, DG_COUNT = 0, 1, 2, 3, 4, 5, 6
DG_NAMES = ('mean', 'var', 'rhat', 'ess', 'mcse', 'ess_sq')
# enum epx_rank_diag (include/epx.h): the columns of a rank-normalised record
RD_RHAT, RD_RHAT_BULK, RD_RHAT_FOLD, RD_ESS_BULK, RD_ESS_TAIL, RD_COUNT = 0, 1, 2, 3, 4, 5
RD_NAMES = ('rhat_rank', 'rhat_bulk', 'rhat_folded', 'ess_bulk', 'ess_tail')
RD_MAX_DRAWS = 8140            # EPX_RD_MAX_DRAWS (include/epx.h): used draws per site the kernel k_rank_diag takes


def split_halves(theta_k, chains):
    """(M, h, P): the M = 2 chains half chains of a site's chain-major draws (S, P); h = nkeep // 2, an odd nkeep drops
    the middle draw."""
    theta_k = np.asarray(theta_k, dtype=np.float64)
    if theta_k.ndim != 2 or chains < 1 or theta_k.shape[0] % chains:
        raise ValueError("theta_k: (S, P) draws with S a multiple of chains = {}".format(chains))
    S, P = theta_k.shape
    nkeep = S // chains
    h = nkeep // 2
    x = theta_k.reshape(chains, nkeep, P)
    return np.stack([x[:, :h], x[:, nkeep - h:]], axis=1).reshape(2 * chains, h, P)


def _geyer(x):
    """(MEAN, var_plus, W, ESS), each (P), of half chains x (M, h, P), h >= 2: Geyer's initial positive, monotone
    sequence over pairs of lags.  ESS is NaN where W is not a finite number > 0."""
    M, h, P = x.shape
    n = M * h
    hm = x.mean(axis=1)                                      # (M, P)
    dev = x - hm[:, None, :]                                 # centred in a second pass

    def acov(t):                                             # mean over the half chains of acov_m(t)
        return (dev[:, :h - t] * dev[:, t:]).sum(axis=1).mean(axis=0) / h

    mean = hm.mean(axis=0)
    W = acov(0) * h / (h - 1)
    var_plus = W * (h - 1) / h + hm.var(axis=0, ddof=1)
    ok = np.isfinite(W) & (W > 0)
    pairs = np.zeros(P)
    prev = np.full(P, np.inf)
    live = ok.copy()
    t = 0
    while t + 1 < h and live.any():
        rho0 = 1.0 if t == 0 else 1.0 - (W - acov(t)) / var_plus
        p = rho0 + (1.0 - (W - acov(t + 1)) / var_plus)
        live &= p > 0                                        # ends in front of the first pair that is not > 0
        p = np.minimum(p, prev)
        prev = np.where(live, p, prev)
        pairs += np.where(live, p, 0.0)
        t += 2
    tau = np.maximum(-1.0 + 2.0 * pairs, 1.0 / np.log10(n))
    return mean, var_plus, W, np.where(ok, n / tau, np.nan)


def diagnostics_host(theta_k, chains):
    """Diagnostics record (P, DG_COUNT) of ONE site from its chain-major draws theta_k (S, P), S = chains x nkeep;
    columns DG_MEAN, DG_VAR, DG_RHAT, DG_ESS, DG_MCSE, DG_ESS_SQ as include/epx.h defines them.  RHAT, ESS, MCSE and
    ESS_SQ are NaN when nkeep < 4 and for a coordinate that is constant or holds a non-finite draw; MEAN and VAR are
    then what the arithmetic gives."""
    x = split_halves(theta_k, chains)
    M, h, P = x.shape
    out = np.full((P, DG_COUNT), np.nan)
    with np.errstate(all='ignore'):
        if h < 2:
            if h == 1:
                out[:, DG_MEAN] = x[:, 0, :].mean(axis=0)    # (W = 0 / 0: nothing else is defined)
            return out
        mean, var_plus, W, ess = _geyer(x)
        _, _, _, ess_sq = _geyer(np.square(x - mean))
        ok = np.isfinite(ess)
        out[:, DG_MEAN] = mean
        out[:, DG_VAR] = var_plus
        out[:, DG_RHAT] = np.where(ok, np.sqrt(var_plus / W), np.nan)
        out[:, DG_ESS] = ess
        out[:, DG_MCSE] = np.where(ok, np.sqrt(var_plus / ess), np.nan)
        out[:, DG_ESS_SQ] = np.where(ok, ess_sq, np.nan)
    return out


def _type7(x, probs):
    """(len(probs), ...) type-7 quantiles along axis 0 of x (n, ...) in the evaluation form of include/epx.h."""
    ranks, plan = _quantiles.rank_plan(x.shape[0], probs)
    return _quantiles.interpolate(_quantiles.order_stats(x, ranks), ranks, plan)


def rank_normalize_host(x, fold=False):
    """(rank, z), each shaped like x: along the LAST axis of x (..., n) the 1-based rank of every value, ties -- equal
    values, -0.0 and +0.0 among them -- at the average rank of their run, and the normal scores
    z = ndtri((rank - 3/8) / (n + 1/4)).  fold: of |x - median| (type 7) instead of x.  A series with a non-finite value
    is NaN throughout.  What k_rank_diag's ranking stage and epx_rank_normalize compute (include/epx.h, enum
    epx_rank_diag)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    flat = x.reshape(-1, n)
    rank = np.full(flat.shape, np.nan)
    for i, v in enumerate(flat):
        if not np.all(np.isfinite(v)):
            continue
        if fold:
            with np.errstate(over='ignore', invalid='ignore'):
                v = np.abs(v - _type7(v, [0.5])[0])
        _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
        rank[i] = (np.cumsum(cnt) - (cnt - 1) / 2.0)[inv.ravel()]     # the run's last rank less half its length - 1
    return rank.reshape(x.shape), ndtri((rank - 0.375) / (n + 0.25)).reshape(x.shape)


def rank_diagnostics_host(theta_k, chains):
    """Rank-normalised record (P, RD_COUNT) of ONE site from its chain-major draws theta_k (S, P), S = chains x nkeep;
    columns RD_RHAT, RD_RHAT_BULK, RD_RHAT_FOLD, RD_ESS_BULK, RD_ESS_TAIL as include/epx.h (enum epx_rank_diag) defines
    them, Rhat and ESS being `_geyer`'s.  All five are NaN when nkeep < 4, for a coordinate with a non-finite draw and
    where the scores have no finite W > 0."""
    x = split_halves(theta_k, chains)
    M, h, P = x.shape
    out = np.full((P, RD_COUNT), np.nan)
    if h < 2 or P == 0:
        return out
    flat = x.reshape(M * h, P)
    good = np.isfinite(flat).all(axis=0)
    x = np.where(good, x, 0.0)                               # (a column of zeros: NaN below, like any constant one)
    flat = x.reshape(M * h, P)
    with np.errstate(all='ignore'):
        q05, q95 = _type7(flat, [0.05, 0.95])
        _, vp, W, ess_bulk = _geyer(rank_normalize_host(flat.T)[1].T.reshape(M, h, P))
        _, vpf, Wf, ess_fold = _geyer(rank_normalize_host(flat.T, fold=True)[1].T.reshape(M, h, P))
        tail = np.minimum(_geyer((x <= q05).astype(np.float64))[3], _geyer((x <= q95).astype(np.float64))[3])
        bulk = np.sqrt(vp / W)
        fold = np.where(np.isfinite(ess_fold), np.sqrt(vpf / Wf), np.nan)
        out[:, RD_RHAT] = np.maximum(bulk, fold)             # (NaN where either is)
        out[:, RD_RHAT_BULK] = bulk
        out[:, RD_RHAT_FOLD] = fold
        out[:, RD_ESS_BULK] = ess_bulk
        out[:, RD_ESS_TAIL] = tail
    out[~(good & np.isfinite(ess_bulk))] = np.nan
    return out


def summarise(rec, n, rank_rec=None):
    """The dict `Master.diagnostics` returns from the records rec (K, Pmax, DG_COUNT) of all sites (NaN behind a site's
    own coordinates) and the used draws per site n (K).  rank_rec (K, Pmax, RD_COUNT): the rank-normalised records; they
    add `rhat_rank`, `rhat_bulk`, `rhat_folded`, `ess_bulk`, `ess_tail`, `site_max_rhat_rank` (NaN entries skipped; NaN
    when all are) and `site_min_ess_rank` (the smallest of `ess_bulk` and `ess_tail`) and change nothing else."""
    out = {name: np.ascontiguousarray(rec[:, :, i]) for i, name in enumerate(DG_NAMES)}
    out['n'] = np.asarray(n, dtype=np.int64)
    with np.errstate(invalid='ignore'):
        rmax = np.where(np.isnan(out['rhat']), -np.inf, out['rhat']).max(axis=1)         # np.nanmax per site ...
        both = np.minimum(np.where(np.isnan(out['ess']), np.inf, out['ess']),
                          np.where(np.isnan(out['ess_sq']), np.inf, out['ess_sq']))      # (K, Pmax): min(ess, ess_sq)
    emin = both.min(axis=1)
    out['site_max_rhat'] = np.where(np.isinf(rmax) & (rmax < 0), np.nan, rmax)           # ... NaN where all are NaN
    out['site_min_ess'] = np.where(np.isinf(emin), np.nan, emin)
    out['worst'] = None
    if not np.isinf(emin).all():
        k = int(np.argmin(emin))
        out['worst'] = (k, int(np.argmin(both[k])))
    if rank_rec is not None:
        out.update((name, np.ascontiguousarray(rank_rec[:, :, i])) for i, name in enumerate(RD_NAMES))
        rmax = np.where(np.isnan(out['rhat_rank']), -np.inf, out['rhat_rank']).max(axis=1)
        emin = np.minimum(np.where(np.isnan(out['ess_bulk']), np.inf, out['ess_bulk']),
                          np.where(np.isnan(out['ess_tail']), np.inf, out['ess_tail'])).min(axis=1)
        out['site_max_rhat_rank'] = np.where(np.isinf(rmax), np.nan, rmax)
        out['site_min_ess_rank'] = np.where(np.isinf(emin), np.nan, emin)
    return out
