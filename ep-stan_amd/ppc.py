"""Posterior predictive checks of the fitted site models on the rows they were fitted to, from the tilted draws: the
responses are replicated from every draw and a statistic of the replicated data is compared with the same statistic of the
observed data, group by group.  This is the NumPy statement of the definition at `enum epx_ppc` (include/epx.h), which the
device kernels k_ppc / k_ppc_sites (csrc/ppc.inc) follow: the expectation of their tests, and `Master.ppc`'s route on an
engine without `replicated_checks`.

The replicates come from the counter-based Philox4x32-10 stream of the samplers (csrc/epx_device.h; newgroup.py holds its
NumPy twin), kind K_PPC: a replicate depends on (seed, row, draw) only, `row` counted over ALL rows of ALL ranks.

A site's draws come from its TILTED distribution, EP's approximation of the posterior of that site's parameters; the check
is conditional on that approximation (see `Master.ppc`).
"""

import numpy as np

from . import newgroup as _newgroup
from . import site_params as _site_params

K_PPC = 7                                                # the stream's kind, next to K_NEWGROUP = 6 (csrc/epx_kernels.h)

# enum epx_ppc (include/epx.h): the columns of a unit's record
PC_T_OBS, PC_T_MEAN, PC_T_M2, PC_T_GE, PC_T_GT, PC_D_OBS_MEAN, PC_D_REP_MEAN, PC_D_LE, PC_COUNT = 0, 1, 2, 3, 4, 5, 6, 7, 8
# the per-draw values of a unit
PD_T_REP, PD_D_OBS, PD_D_REP = 0, 1, 2

_TWO_PI = 6.283185307179586476925286766559


def _stream_rows(rows):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    if rows.size and (rows.min() < 0 or rows.max() >= 2 ** 32):
        raise ValueError("rows of the stream outside [0, 2^32)")
    return rows


def replicate_uniforms(seed, rows, S):
    """u1 (S, n) of the Bernoulli family's replicates: the first uniform of counter (s, K_PPC, row, 0) under key
    (seed, 0)."""
    rows = _stream_rows(rows)
    s = np.arange(S, dtype=np.uint64)[:, None]
    return _newgroup.rng_u2(_newgroup.make_key(seed, 0), s, K_PPC, rows.astype(np.uint64)[None, :], 0)[0]


def replicate_normals(seed, rows, S, dtype=np.float64, kind=K_PPC):
    """z (S, n) of the Gaussian family's replicates: csrc/epx_device.h rng_normal(key, s, kind, e = row, 0) restated --
    the Box-Muller pair of counter (s, kind, e >> 1, 0), e the row as a 32-bit signed integer, cosine for even e.  The
    uniforms are the stream's doubles; the logarithm, root, sine and cosine are taken in `dtype`.  kind: K_PPC, or the
    stream kind of another entry that replicates responses this way (predict_quantiles.K_PRED_REP)."""
    rows = _stream_rows(rows)
    e = rows.astype(np.uint32).view(np.int32)
    a = (e >> 1).astype(np.int64) & 0xFFFFFFFF
    s = np.arange(S, dtype=np.uint64)[:, None]
    u1, u2 = _newgroup.rng_u2(_newgroup.make_key(seed, 0), s, kind, a.astype(np.uint64)[None, :], 0)
    dt = np.dtype(dtype).type
    u1, u2 = u1.astype(dtype), u2.astype(dtype)
    rad = np.sqrt(dt(-2) * np.log(u1))
    two_pi = dt(_TWO_PI) if np.dtype(dtype) == np.float64 else dt(8) * np.arctan(dt(1))      # (2 pi of the wider type)
    ang = two_pi * u2
    return np.where((rows & 1).astype(bool)[None, :], rad * np.sin(ang), rad * np.cos(ang))


def sigmoid(f):
    """sigmoid(f) through exp(-|f|), as site_params.predict_host forms it."""
    e = np.exp(-np.abs(f))
    return np.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _loglik(gauss, ls, f, y):
    """site_params.loglik_of in float64; the same expressions in the dtype of f otherwise.  ls (S, 1): log sigma."""
    if f.dtype == np.float64:
        return _site_params.loglik_of(gauss, ls, f, y)
    dt = f.dtype.type
    y = np.asarray(y).astype(f.dtype)
    if gauss:
        ls = ls.astype(f.dtype)
        return -dt(0.5) * np.log(dt(2) * (dt(4) * np.arctan(dt(1)))) - ls - dt(0.5) * np.square((y - f) / np.exp(ls))
    return y * f - (np.maximum(f, dt(0)) + np.log1p(np.exp(-np.abs(f))))


def site_cells(model_id, D, ng, gauss, theta, X, group, y, seed, rows, dtype=np.float64):
    """(f, y_rep, ll_obs, ll_rep), (S, n) each, of the rows X (n, D), y (n) of ONE site under its draws theta (S, P).
    group (n): the 0-based group of every row within the site (None: 0); rows (n): every row's index in the stream.  f is
    site_params.linear_predictor's (float64); the link, the normals and the log-likelihoods are taken in `dtype`."""
    theta = np.asarray(theta, dtype=np.float64)
    S = theta.shape[0]
    f = _site_params.linear_predictor(model_id, D, ng, gauss, theta, X, group).astype(dtype)
    ls = theta[:, :1]
    with np.errstate(all='ignore'):
        if gauss:
            y_rep = f + np.exp(ls.astype(dtype)) * replicate_normals(seed, rows, S, dtype)
        else:
            y_rep = (replicate_uniforms(seed, rows, S) < sigmoid(f)).astype(dtype)
        yv = np.asarray(y, dtype=np.float64)
        return f, y_rep, _loglik(gauss, ls, f, yv), _loglik(gauss, ls, f, y_rep)


def site_per_draw(model_id, D, ng, gauss, theta, X, group, y, seed, rows, dtype=np.float64):
    """(per_draw (ng, 3, S), t_obs (ng), bad (ng)) of ONE site: T_rep, D_obs, D_rep of every (group, draw), the groups'
    sums of y, and whether a group holds a cell with a non-finite f, ll(y) or ll(y_rep).  Arguments as `site_cells`.
    D_obs and D_rep are added over the same rows in the same order."""
    n = np.asarray(X).reshape(-1, D).shape[0]
    group = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    f, y_rep, ll_obs, ll_rep = site_cells(model_id, D, ng, gauss, theta, X, group, y, seed, rows, dtype)
    S = f.shape[0]
    per_draw = np.zeros((ng, 3, S), dtype=dtype)
    t_obs, bad = np.zeros(ng, dtype=dtype), np.zeros(ng, dtype=bool)
    yv = np.asarray(y).astype(dtype)
    for g in range(ng):
        at = np.nonzero(group == g)[0]
        per_draw[g, PD_T_REP] = y_rep[:, at].sum(axis=1)
        per_draw[g, PD_D_OBS] = ll_obs[:, at].sum(axis=1)
        per_draw[g, PD_D_REP] = ll_rep[:, at].sum(axis=1)
        t_obs[g] = yv[at].sum()
        bad[g] = not (np.all(np.isfinite(f[:, at])) and np.all(np.isfinite(ll_obs[:, at]))
                      and np.all(np.isfinite(ll_rep[:, at])))
    return per_draw, t_obs, bad


def record(per_draw, t_obs, bad=False):
    """The eight numbers of `enum epx_ppc` of ONE unit from its per-draw values (3, S); NaN in all for a `bad` unit."""
    per_draw = np.asarray(per_draw)
    out = np.full(PC_COUNT, np.nan, dtype=per_draw.dtype)
    if bad:
        return out
    S = per_draw.shape[1]
    t, d_obs, d_rep = per_draw
    mean = t.sum() / S
    out[PC_T_OBS] = t_obs
    out[PC_T_MEAN] = mean
    out[PC_T_M2] = np.square(t - mean).sum()             # centred: never sum t^2 - S mean^2
    out[PC_T_GE] = np.count_nonzero(t >= t_obs)
    out[PC_T_GT] = np.count_nonzero(t > t_obs)
    out[PC_D_OBS_MEAN] = d_obs.sum() / S
    out[PC_D_REP_MEAN] = d_rep.sum() / S
    out[PC_D_LE] = np.count_nonzero(d_rep <= d_obs)
    return out


def site_records(per_draw, t_obs, bad):
    """(groups (ng, 8), site (8), per_draw (ng, 3, S)) of ONE site from `site_per_draw`'s result.  The site's per-draw
    values are its groups', added in group order; a bad group makes the site bad."""
    groups = np.stack([record(per_draw[g], t_obs[g], bad[g]) for g in range(per_draw.shape[0])])
    tot, tt = per_draw[0].copy(), t_obs[0]
    for g in range(1, per_draw.shape[0]):
        tot, tt = tot + per_draw[g], tt + t_obs[g]
    return groups, record(tot, tt, bool(np.any(bad))), per_draw


def ppc_host(model_id, D, site_ng, gauss, thetas, X, group, y, k_lim, seed=0, row0=0, dtype=np.float64):
    """(groups (G, 8), sites (K, 8), draws (G, 3, S)) of K sites: thetas[k] (S, P) the draws of site k, whose rows are
    k_lim[k]..k_lim[k+1] of X (N, D), y (N); site_ng (K): the groups of every site; group (N): the 0-based group of every
    row within its site (None: one group per site); the stream's row of row i is row0 + i."""
    K = len(site_ng)
    groups, sites, draws = [], [], []
    for k in range(K):
        lo, hi = int(k_lim[k]), int(k_lim[k + 1])
        g, s, d = site_records(*site_per_draw(
            model_id, D, int(site_ng[k]), gauss, thetas[k], X[lo:hi], None if group is None else group[lo:hi], y[lo:hi],
            seed, row0 + np.arange(lo, hi, dtype=np.int64), dtype))
        groups.append(g)
        sites.append(s)
        draws.append(d)
    return np.concatenate(groups), np.stack(sites), np.concatenate(draws)


def _unit_summary(rec, S, prefix):
    rec = np.asarray(rec, dtype=np.float64)
    return {prefix + 't_obs': rec[:, PC_T_OBS].copy(),
            prefix + 't_rep_mean': rec[:, PC_T_MEAN].copy(),
            prefix + 't_rep_var': rec[:, PC_T_M2] / (S - 1) if S > 1 else np.full(rec.shape[0], np.nan),
            prefix + 'p_t_ge': rec[:, PC_T_GE] / S,
            prefix + 'p_t': (rec[:, PC_T_GE] + rec[:, PC_T_GT]) / (2.0 * S),
            prefix + 'd_obs_mean': rec[:, PC_D_OBS_MEAN].copy(),
            prefix + 'd_rep_mean': rec[:, PC_D_REP_MEAN].copy(),
            prefix + 'p_d': rec[:, PC_D_LE] / S}


def summarise(groups, sites, S, site_ng, level=0.05, draws=None):
    """The result of `Master.ppc` from the records of all groups (G, 8) and sites (K, 8) over S draws per site; site_ng
    (K): the groups of every site.  Returns a dict: per group (G each) `group_site`, `t_obs`, `t_rep_mean`, `t_rep_var`
    = T_M2 / (S - 1), `p_t_ge` = T_GE / S, `p_t` = (T_GE + T_GT) / (2 S) (the mid-p), `d_obs_mean`, `d_rep_mean`, `p_d` =
    D_LE / S; per site (K each) the same under `site_*`; `n` = S; `level`; `extreme`: the indices of the groups whose `p_t`
    or `p_d` lies outside [level / 2, 1 - level / 2] (a NaN group is not among them); `draws` (G, 3, S) where given."""
    if not 0.0 < level < 1.0:
        raise ValueError("`level` must lie in (0, 1)")
    S = int(S)
    site_ng = np.asarray(site_ng, dtype=np.int64)
    out = dict(n=S, level=float(level), group_site=np.repeat(np.arange(site_ng.shape[0]), site_ng))
    out.update(_unit_summary(groups, S, ''))
    out.update(_unit_summary(sites, S, 'site_'))
    lo, hi = level / 2.0, 1.0 - level / 2.0
    with np.errstate(invalid='ignore'):
        far = (out['p_t'] < lo) | (out['p_t'] > hi) | (out['p_d'] < lo) | (out['p_d'] > hi)
    out['extreme'] = np.nonzero(far)[0]
    if draws is not None:
        out['draws'] = draws
    return out
