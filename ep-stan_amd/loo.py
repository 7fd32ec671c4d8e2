"""Leave-one-out cross-validation of the fitted site models from the tilted draws: PSIS-LOO (Pareto-smoothed importance
sampling; Vehtari, Simpson, Gelman, Yao & Gabry) with its Pareto k-hat diagnostic, and WAIC.  This is the NumPy / SciPy
statement of the definition at `enum epx_loo` (include/epx.h), which the device kernels k_loo (csrc/predict.hip) and
k_psis_rows with csrc/psis.h follow: the expectation of their tests, and `Master.loo`'s route on an engine without `loo`.

A site's draws come from its TILTED distribution, EP's approximation of the posterior of that site's parameters; the
leave-one-out is conditional on that approximation (see `Master.loo`).
"""

import math

import numpy as np

from . import site_params as _site_params

# enum epx_loo (include/epx.h): the columns of a leave-one-out record
LO_LPD, LO_LL_MEAN, LO_LL_M2, LO_ELPD, LO_KHAT, LO_WESS, LO_COUNT = 0, 1, 2, 3, 4, 5, 6

MIN_TAIL = 5            # a shorter tail is not smoothed


def tail_length(S):
    """M = min(floor(S / 5), ceil(3 sqrt(S))) in integers."""
    c = math.isqrt(9 * S)
    return min(S // 5, c if c * c == 9 * S else c + 1)


def _logsumexp(v):
    top = v.max()
    return top + np.log(np.exp(v - top).sum())


def gpd_fit(x):
    """Zhang & Stephens' estimate of the generalised Pareto distribution of the excesses x (M, ascending, the largest
    positive): (khat, sigma), khat with the weakly informative prior of ten pseudo-observations at 0.5,
    (M k + 5) / (M + 10), and sigma = -k / b from the k before the prior.  Works in the dtype of x."""
    x = np.asarray(x)
    dt = x.dtype.type
    M = x.shape[0]
    m = 30 + math.isqrt(M)
    xq = x[int(math.floor(M / 4 + 0.5)) - 1]
    i = np.arange(1, m + 1).astype(x.dtype)
    b = dt(1) / x[-1] + (dt(1) - np.sqrt(dt(m) / (i - dt(0.5)))) / (dt(3) * xq)
    k = np.log1p(-b[:, None] * x[None, :]).mean(axis=1)
    L = dt(M) * (np.log(-b / k) - k - dt(1))
    w = dt(1) / np.exp(L[None, :] - L[:, None]).sum(axis=1)
    bb = (b * w).sum()
    k = np.log1p(-bb * x).mean()
    sigma = -k / bb
    return (dt(M) * k + dt(5)) / dt(M + 10), sigma


def _psis_row(ll):
    """(ELPD, KHAT, WESS) of ONE row's log-likelihoods ll (S), in the dtype of ll."""
    dt = ll.dtype.type
    S = ll.shape[0]
    if not np.all(np.isfinite(ll)):
        return dt(np.nan), dt(np.nan), dt(np.nan)
    lr = -ll - (-ll).max()
    M = tail_length(S)
    khat = dt(np.inf)
    if M >= MIN_TAIL:
        order = np.argsort(lr, kind='stable')            # ascending by (lr, draw index)
        tail = order[S - M:]
        eu = np.exp(lr[order[S - M - 1]])
        x = np.exp(lr[tail]) - eu
        xq = x[int(math.floor(M / 4 + 0.5)) - 1]
        if xq > 0 and x[-1] > xq:
            with np.errstate(all='ignore'):
                k, sigma = gpd_fit(x)
            if np.isfinite(k):
                p = (np.arange(1, M + 1).astype(ll.dtype) - dt(0.5)) / dt(M)
                if k == 0:
                    q = -sigma * np.log1p(-p)
                else:
                    q = (sigma / k) * np.expm1(-k * np.log1p(-p))
                lr = lr.copy()
                with np.errstate(all='ignore'):
                    lr[tail] = np.minimum(dt(0), np.log(eu + q))
                khat = k
    lw = lr - _logsumexp(lr)
    return _logsumexp(lw + ll), khat, dt(1) / np.exp(dt(2) * lw).sum()


def psis_host(ll):
    """PSIS of every row of ll (n, S), the log-likelihoods of n rows under S draws: (n, 3), columns ELPD, KHAT, WESS as
    `enum epx_loo` defines them.  Works in the dtype of ll (float64, or np.longdouble for the tests' error scale)."""
    ll = np.asarray(ll)
    if ll.dtype != np.longdouble:
        ll = ll.astype(np.float64)
    if ll.ndim != 2 or ll.shape[1] < 1:
        raise ValueError('ll: (n, S) with S >= 1')
    out = np.empty((ll.shape[0], 3), dtype=ll.dtype)
    for i in range(ll.shape[0]):
        out[i] = _psis_row(ll[i])
    return out


def loo_rows(ll):
    """The six numbers of `enum epx_loo` for every row of ll (n, S): (n, 6)."""
    ll = np.asarray(ll, dtype=np.float64)
    n, S = ll.shape
    out = np.full((n, LO_COUNT), np.nan)
    ok = np.all(np.isfinite(ll), axis=1)
    if ok.any():
        v = ll[ok]
        top = v.max(axis=1)
        out[ok, LO_LPD] = top + np.log(np.exp(v - top[:, None]).mean(axis=1))
        mean = v.mean(axis=1)
        out[ok, LO_LL_MEAN] = mean
        out[ok, LO_LL_M2] = np.square(v - mean[:, None]).sum(axis=1)
        out[ok, LO_ELPD:] = psis_host(v)
    return out


def loglik_host(model_id, D, ng, gauss, theta, X, group, y):
    """ll (n, S): the log-likelihood of every row's response under every draw theta (S, P) of ONE site."""
    f = _site_params.linear_predictor(model_id, D, ng, gauss, theta, X, group)
    return np.ascontiguousarray(_site_params.loglik_of(gauss, theta, f, y).T)


def loo_host(model_id, D, ng, gauss, theta, X, group, y):
    """Leave-one-out records (n, 6) of the rows X (n, D), y (n) of ONE site from its draws theta (S, P); group (n): the
    0-based group of every row within the site (None: 0)."""
    return loo_rows(loglik_host(model_id, D, ng, gauss, theta, X, group, y))


def khat_threshold(S):
    """min(1 - 1 / log10(S), 0.7): above it a row's leave-one-out estimate is not reliable at S draws."""
    return min(1.0 - 1.0 / math.log10(S), 0.7) if S > 1 else -math.inf


def summarise(rec, S, k_lim):
    """The model-comparison summary of the records rec (N, 6) of all rows (S draws per site, the rows of site k are
    k_lim[k]..k_lim[k+1]).  Returns a dict:
      elpd_loo, p_loo = sum (LPD - ELPD), elpd_waic = sum (LPD - LL_M2 / (S - 1)), p_waic: the totals;
      se_elpd_loo, se_p_loo, se_elpd_waic, se_p_waic: sqrt(N var(pointwise, ddof=1));
      lpd, elpd_loo_i, p_loo_i, elpd_waic_i, p_waic_i, khat, wess, ll_mean (N each): pointwise;
      site_elpd_loo, site_p_loo, site_elpd_waic, site_p_waic, site_lpd (K each): the sums of every site's rows;
      n: S; khat_threshold; n_bad: the rows whose khat exceeds the threshold (+inf, a row that was not smoothed,
      included); worst: (site, row within the site) of the largest finite khat, None when there is none."""
    rec = np.asarray(rec, dtype=np.float64)
    k_lim = np.asarray(k_lim, dtype=np.int64)
    N = rec.shape[0]
    lpd, khat = rec[:, LO_LPD].copy(), rec[:, LO_KHAT].copy()
    p_waic = rec[:, LO_LL_M2] / (S - 1) if S > 1 else np.full(N, np.nan)
    point = dict(elpd_loo=rec[:, LO_ELPD].copy(), p_loo=lpd - rec[:, LO_ELPD], elpd_waic=lpd - p_waic, p_waic=p_waic)
    out = dict(n=int(S), lpd=lpd, khat=khat, wess=rec[:, LO_WESS].copy(), ll_mean=rec[:, LO_LL_MEAN].copy())
    starts = k_lim[:-1] - k_lim[0]
    for name, v in point.items():
        out[name] = float(v.sum())
        out['se_' + name] = float(np.sqrt(N * v.var(ddof=1))) if N > 1 else float('nan')
        out[name + '_i'] = v
        out['site_' + name] = np.add.reduceat(v, starts) if N else np.zeros(0)
    out['site_lpd'] = np.add.reduceat(lpd, starts) if N else np.zeros(0)
    thr = khat_threshold(S)
    out['khat_threshold'] = thr
    out['n_bad'] = int(np.count_nonzero(khat > thr))
    finite = np.nonzero(np.isfinite(khat))[0]
    out['worst'] = None
    if finite.size:
        i = int(finite[np.argmax(khat[finite])])
        k = int(np.searchsorted(k_lim - k_lim[0], i, side='right') - 1)
        out['worst'] = (k, i - int(k_lim[k] - k_lim[0]))
    return out
