"""Predictive intervals of new rows from order statistics across draws (`Master.predict_quantiles`), in plain NumPy.

The definition is stated at `enum epx_pred_order` (include/epx.h): per new row the value v = f (the linear predictor) or
f + sigma z (the replicated response of the Gaussian family) of every draw of the row's site, ordered by key; the device
kernel k_predict_order (csrc/predict_order.inc) delivers ORDER STATISTICS and the host interpolates, as for
`Master.mix_quantiles`.  This module holds the host restatement of the device's share (`predict_order_stats_host`: the
expectation of the kernel's tests and `Master.predict_quantiles`' route on an engine without `predict_order_stats`) and
the host's own share (`stable_sigmoid`, `quantiles_of`).

The replicates come from the counter-based Philox4x32-10 stream of the samplers at kind K_PRED_REP: a replicate depends
on (seed, row_id, draw) only."""

import numpy as np

from . import ppc as _ppc
from . import quantiles as _quantiles
from . import site_params as _site_params

K_PRED_REP = 9                                           # the stream's kind, next to K_BRIDGE = 8 (csrc/epx_kernels.h)
PO_F, PO_YREP = 0, 1                                     # enum epx_pred_order (include/epx.h)
WHAT = {'f': PO_F, 'yrep': PO_YREP}
SCALES = ('linear', 'mean', 'response')


def what_id(what, gauss):
    """enum epx_pred_order of `what` ('f', 'yrep'); 'yrep' is the Gaussian family's."""
    if what not in WHAT:
        raise ValueError("what: one of {} (got {!r})".format(sorted(WHAT), what))
    if what == 'yrep' and not gauss:
        raise ValueError("what = 'yrep' is defined for the Gaussian family only: a Bernoulli-logit model's 0/1 replicate "
                         "has no useful quantile")
    return WHAT[what]


def site_values(model_id, D, ng, gauss, theta, Xn, group, what='f', seed=0, row_id=None, dtype=np.float64):
    """v (S, n) of the rows Xn (n, D) of ONE site under its draws theta (S, P): f of site_params.linear_predictor
    (float64), or with what = 'yrep' f + exp(phi[0]) z, z ppc.replicate_normals at kind K_PRED_REP of the rows' stream
    indices row_id (n); the exponential, the normals and the sum are taken in `dtype`."""
    what_id(what, gauss)
    theta = np.asarray(theta, dtype=np.float64)
    f = _site_params.linear_predictor(model_id, D, ng, gauss, theta, Xn, group).astype(dtype)
    if what == 'f':
        return f
    with np.errstate(all='ignore'):
        z = _ppc.replicate_normals(seed, row_id, theta.shape[0], dtype, kind=K_PRED_REP)
        return f + np.exp(theta[:, :1].astype(dtype)) * z


def predict_order_stats_host(model_id, D, site_ng, gauss, thetas, Xn, row_lim, ranks, row_group=None, what='f', seed=0,
                             row_id=None, dtype=np.float64):
    """(n, len(ranks)): the order statistics v_(r), r in ranks, of every new row's values over the draws of its site.
    thetas[j] (S, P): the draws of site j, whose rows are row_lim[j]..row_lim[j+1] of Xn (n, D); site_ng: the groups of
    every site; row_group (n): 0-based group of every row within its site (None: 0); row_id (n): the rows' stream indices
    (None: the row's position in the call).  A row with a NaN value has NaN at every rank.  What k_predict_order
    computes; in a wider `dtype` the values are rounded to float64 before they are ordered."""
    Xn = np.asarray(Xn, dtype=np.float64).reshape(-1, D)
    n = Xn.shape[0]
    ranks = np.asarray(ranks, dtype=np.int64).ravel()
    row_id = np.arange(n, dtype=np.int64) if row_id is None else np.asarray(row_id, dtype=np.int64)
    out = np.zeros((n, ranks.size))
    for j in range(len(site_ng)):
        lo, hi = int(row_lim[j]), int(row_lim[j + 1])
        if hi > lo:
            v = site_values(model_id, D, int(site_ng[j]), gauss, thetas[j], Xn[lo:hi],
                            None if row_group is None else row_group[lo:hi], what, seed, row_id[lo:hi], dtype)
            out[lo:hi] = _quantiles.order_stats(v.astype(np.float64), ranks).T
    return out


def stable_sigmoid(f):
    """sigmoid(f) through exp(-|f|): no overflow at either end, monotone, NaN for NaN."""
    f = np.asarray(f, dtype=np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.exp(-np.abs(f))
        return np.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def quantiles_of(stats, ranks, plan, through_sigmoid):
    """(len(plan), n) quantiles from the rows' order statistics stats (n, len(ranks)) of `quantiles.rank_plan`'s ranks.
    through_sigmoid: the order statistics of f are mapped through the sigmoid first -- the map is monotone, so these are
    the order statistics, and the type-7 quantiles, of sigmoid(f)."""
    stats = np.asarray(stats, dtype=np.float64).T
    return _quantiles.interpolate(stable_sigmoid(stats) if through_sigmoid else stats, ranks, plan)
