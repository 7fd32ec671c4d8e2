"""Per-coordinate sampler diagnostics of one site's draws in plain NumPy: split-Rhat, effective sample sizes and the
Monte-Carlo standard error of the tilted mean.  The definition is stated in include/epx.h (enum epx_diag); the device
kernel k_draw_diag (csrc/draw_diag.hip) computes the same next to the draws.  `diagnostics_host` is the expectation of
the kernel's tests and `Master.diagnostics`' route on an engine without `draw_diagnostics`."""

import numpy as np

# enum epx_diag (include/epx.h): the columns of a diagnostics record
DG_MEAN, DG_VAR, DG_RHAT, DG_ESS, DG_MCSE, DG_ESS_SQ, DG_COUNT = 0, 1, 2, 3, 4, 5, 6
DG_NAMES = ('mean', 'var', 'rhat', 'ess', 'mcse', 'ess_sq')


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


def summarise(rec, n):
    """The dict `Master.diagnostics` returns from the records rec (K, Pmax, DG_COUNT) of all sites (NaN behind a site's
    own coordinates) and the used draws per site n (K)."""
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
    return out
