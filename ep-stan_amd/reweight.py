"""Reuse of a site's tilted draws across EP iterations.  Between two iterations a site's tilted distribution changes only
through its Gaussian cavity, so the tilted moments under the new cavity follow from the draws sampled against the old one
by Pareto-smoothed importance sampling, with no likelihood evaluation.  This is the NumPy statement of the definition at
`epx_reweight_batch` (include/epx.h), which the device kernel k_reweight (csrc/dense.hip) follows: the expectation of its
tests; and the acceptance rule `Master.run(reuse=...)` applies to the kernel's records.
"""

import math

import numpy as np

from . import loo as _loo

# enum epx_reweight (include/epx.h): the columns of a site's record
RW_KHAT, RW_WESS, RW_COUNT = 0, 1, 2


def reuse_ok(khat, wess, S, k_max=None, min_ess=0.5):
    """A site's draws may stand in for fresh ones iff wess >= min_ess * S and (khat == +inf or khat <= k_max); khat is
    +inf exactly when the tail was not smoothed, and the effective sample size is then the whole check.  k_max=None:
    loo.khat_threshold(S).  The defaults are policy the caller may override; elementwise over arrays."""
    if k_max is None:
        k_max = _loo.khat_threshold(S)
    khat, wess = np.asarray(khat, dtype=np.float64), np.asarray(wess, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        ok = (wess >= min_ess * S) & (np.isposinf(khat) | (khat <= k_max))
    return bool(ok) if ok.ndim == 0 else ok


def psis_weights(lr):
    """The normalised smoothed log weights of the log ratios lr (S, finite): (lw, khat) exactly as loo._psis_row forms them
    on ll = -lr, in the dtype of lr."""
    dt = lr.dtype.type
    S = lr.shape[0]
    lr = lr - lr.max()
    M = _loo.tail_length(S)
    khat = dt(np.inf)
    if M >= _loo.MIN_TAIL:
        order = np.argsort(lr, kind='stable')
        tail = order[S - M:]
        eu = np.exp(lr[order[S - M - 1]])
        x = np.exp(lr[tail]) - eu
        xq = x[int(math.floor(M / 4 + 0.5)) - 1]
        if xq > 0 and x[-1] > xq:
            with np.errstate(all='ignore'):
                k, sigma = _loo.gpd_fit(x)
            if np.isfinite(k):
                p = (np.arange(1, M + 1).astype(lr.dtype) - dt(0.5)) / dt(M)
                q = -sigma * np.log1p(-p) if k == 0 else (sigma / k) * np.expm1(-k * np.log1p(-p))
                lr = lr.copy()
                with np.errstate(all='ignore'):
                    lr[tail] = np.minimum(dt(0), np.log(eu + q))
                khat = k
    top = lr.max()
    return lr - (top + np.log(np.exp(lr - top).sum())), khat


def precision_host(mean, scatter, n, Q, r, prec_estim):
    """Step 6: the precision estimate from the tilted mean and scatter with n draws' worth, and the site update: (dQi, dri,
    ok), float64.  'sample': inv(scatter) (n - d - 2); 'olse': the oracle-approximating shrinkage of scatter / n towards
    the prior matrix Q.  ok False (and a zero update): the Cholesky fails, or under 'sample' n - d - 2 <= 0."""
    mean, scatter = np.asarray(mean, dtype=np.float64), np.asarray(scatter, dtype=np.float64)
    Q, r = np.asarray(Q, dtype=np.float64), np.asarray(r, dtype=np.float64)
    d, n = mean.shape[0], float(n)
    zero = (np.zeros((d, d)), np.zeros(d), False)
    if prec_estim not in ('sample', 'olse'):
        raise ValueError('Invalid value for option `prec_estim`')
    if not (np.all(np.isfinite(scatter)) and np.isfinite(n)):
        return zero
    if prec_estim == 'sample' and not n - (d + 2) > 0:
        return zero
    A = scatter if prec_estim == 'sample' else scatter / n
    try:
        np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return zero
    A = np.linalg.inv(A)
    A = 0.5 * (A + A.T)
    if prec_estim == 'sample':
        Qt = A * (n - (d + 2))
    else:
        tr, f2, f2p, tsp = np.trace(A), np.sum(A * A), np.sum(Q * Q), np.sum(A * Q)
        alpha = 1.0 - (d + tr * tr * f2p / (f2 * f2p - tsp * tsp)) / n
        beta = (tsp / f2p) * (1.0 - d / n - alpha)
        Qt = alpha * A + beta * Q
    return Qt - Q, Qt.dot(mean) - r, True


def reweight_host(phi, Om_old, mu_old, Om_new, mu_new, Q, r, prec_estim):
    """One site: phi (S, d) draws sampled against the cavity N(mu_old, Om_old^-1), reweighted to N(mu_new, Om_new^-1).
    Works in the dtype of phi (float64, or np.longdouble for the tests' error scale) up to and including the weighted
    moments; the precision estimate is float64.  Returns a dict: mean (d), scatter (d, d), khat, wess, lw (S), lr (S),
    dQi (d, d), dri (d), ok.  A log ratio that is not finite: NaN mean, scatter, khat, wess and lw, a zero update."""
    phi = np.asarray(phi)
    if phi.dtype != np.longdouble:
        phi = phi.astype(np.float64)
    dt = phi.dtype
    Oo, mo, On, mn = (np.asarray(v).astype(dt) for v in (Om_old, mu_old, Om_new, mu_new))
    S, d = phi.shape
    m0 = phi.sum(axis=0) / dt.type(S)
    c = phi - m0
    dOm = On - Oo
    g = On.dot(mn - m0) - Oo.dot(mo - m0)
    with np.errstate(all='ignore'):
        lr = (c * (g - dt.type(0.5) * c.dot(dOm))).sum(axis=1)
    if not np.all(np.isfinite(lr)):
        nan = dt.type(np.nan)
        return dict(mean=np.full(d, nan), scatter=np.full((d, d), nan), khat=nan, wess=nan, lw=np.full(S, nan), lr=lr,
                    dQi=np.zeros((d, d)), dri=np.zeros(d), ok=False)
    lw, khat = psis_weights(lr)
    wess = dt.type(1) / np.exp(dt.type(2) * lw).sum()
    w = np.exp(lw)
    dm = w.dot(c)
    mean = m0 + dm
    cc = c - dm
    scatter = wess * (cc * w[:, None]).T.dot(cc)
    dQi, dri, ok = precision_host(mean.astype(np.float64), scatter.astype(np.float64), float(wess), Q, r, prec_estim)
    return dict(mean=mean, scatter=scatter, khat=khat, wess=wess, lw=lw, lr=lr, dQi=dQi, dri=dri, ok=ok)
