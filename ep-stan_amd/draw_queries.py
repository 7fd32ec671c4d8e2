"""What `Master`'s draw queries -- mix_pred, mix_quantiles, predict, predict_quantiles, predict_new_group, loo, diagnostics
and diagnostics(rank=True): everything answered from the tilted draws the last iteration left on the device -- share, away from
the class that runs EP.  Nothing here knows a `Master`:

  QUERIES, HostDraws, Queries   the eight engine methods behind the queries; the host route to each of them, stated once
                                with `HipEngine`'s argument names and record shapes; and the per-method choice between an
                                engine's own method and the host route
  CHECKS                        the engine method behind `Master.ppc`, on both routes and resolved by the same rule
  INTERVALS                     the engine method behind `Master.predict_quantiles`, likewise
  gather_site_records           the ONLY way per-site records travel between ranks: one flat record per site, padded to the
                                widest site; gather_named_records packs {name: array} records on top of it
  plan_rows                     predict's rows -> sites arithmetic, pure
  sum_predict_rows, sum_loo_rows, sum_order_rows, merge_new_group
                                the four row collectives, each with its own treatment of non-finite values
"""

import numpy as np

from . import diagnostics as _diagnostics
from . import evidence as _evidence
from . import loo as _loo
from . import mix_pred as _mix_pred
from . import newgroup as _newgroup
from . import ppc as _ppc
from . import predict_quantiles as _predict_quantiles
from . import quantiles as _quantiles
from . import site_params as _site_params

QUERIES = ('named_moments', 'pooled_count_pass', 'named_order_stats', 'predict', 'predict_new_group', 'loo',
           'draw_diagnostics', 'draw_rank_diagnostics')
# the engine method behind `Master.ppc`: resolved like QUERIES, kept apart from the eight
CHECKS = ('replicated_checks',)
# the engine method behind `Master.predict_quantiles`: likewise
INTERVALS = ('predict_order_stats',)


class HostDraws(object):
    """The host route of QUERIES: an engine-shaped object over a sampling engine's `get_draws`, for an engine without the
    device methods (the CPU oracle the tests inject).  Every method takes what `Master` passes `HipEngine`'s method of the
    same name and returns its shapes; the arithmetic is the pure modules'.  Nothing is kept between calls.

    engine_of(): the sampling engine at the time of a call (`get_draws`, `num_draws`, `d`, `P`); spec: `engine.site_spec`
    of the site model; of this rank's sites: site_ng the groups of each, X, y, j_ind (1-based, None for an `_sg` model)
    their rows, k_lim the sites' limits in them."""

    def __init__(self, engine_of, spec, D, site_ng, X, y, j_ind, k_lim, chains):
        self.engine_of, self.spec, self.D, self.site_ng, self.K = engine_of, spec, D, site_ng, len(site_ng)
        self.X, self.y, self.j_ind, self.k_lim, self.chains = X, y, j_ind, k_lim, int(chains)

    engine = property(lambda self: self.engine_of())

    def _named_draws(self, names, j):
        """{name: draws} of site j (site_params.named_draws)."""
        mid, gauss, sg = self.spec
        theta = np.ascontiguousarray(self.engine.get_draws(j, all_params=True))
        return _site_params.named_draws(mid, self.D, int(self.site_ng[j]), gauss, sg, theta, names)

    def named_moments(self, names):
        mid, gauss, sg = self.spec
        n, means, m2s = 0, [], []
        for j in range(self.K):
            theta = self.engine.get_draws(j, all_params=True)
            n, m, v = _site_params.named_moments_host(mid, self.D, int(self.site_ng[j]), gauss, sg, theta, names)
            means.append(m)
            m2s.append(v)
        return n, means, m2s

    def pooled_count_pass(self, names, shift, prefix, n_targets):
        x = np.concatenate([np.concatenate([d[name].reshape(d[name].shape[0], -1) for name in names], axis=1)
                            for d in (self._named_draws(names, j) for j in range(self.K))])
        return _quantiles.count_pass_host(x, shift, prefix, n_targets)

    def named_order_stats(self, names, ranks):
        return [dict((name, _quantiles.order_stats(d[name], ranks)) for name in names)
                for d in (self._named_draws(names, j) for j in range(self.K))]

    def predict(self, Xn, row_lim, row_group=None, y=None):
        mid, gauss, _ = self.spec
        out = np.zeros((Xn.shape[0], _site_params.PR_COUNT))
        for j in range(self.K):
            lo, hi = int(row_lim[j]), int(row_lim[j + 1])
            if hi > lo:
                out[lo:hi] = _site_params.predict_host(
                    mid, self.D, int(self.site_ng[j]), gauss, self.engine.get_draws(j, all_params=True), Xn[lo:hi],
                    None if row_group is None else row_group[lo:hi], None if y is None else y[lo:hi])
        return out

    def predict_order_stats(self, Xn, row_lim, ranks, row_group=None, what='f', seed=0, row_id=None, with_n=False):
        mid, gauss, _ = self.spec
        _predict_quantiles.what_id(what, gauss)
        out = np.zeros((Xn.shape[0], len(ranks)))
        for j in range(self.K):                          # a site's draws are fetched where it has rows, one site at a time
            lo, hi = int(row_lim[j]), int(row_lim[j + 1])
            if hi > lo:
                out[lo:hi] = _predict_quantiles.predict_order_stats_host(
                    mid, self.D, self.site_ng[j:j + 1], gauss, [self.engine.get_draws(j, all_params=True)], Xn[lo:hi],
                    [0, hi - lo], ranks, None if row_group is None else row_group[lo:hi], what, seed,
                    np.arange(lo, hi, dtype=np.int64) if row_id is None else row_id[lo:hi])
        return (out, int(self.engine.num_draws())) if with_n else out

    def predict_new_group(self, Xn, gidx, labels, y=None, seed=0, t0=0, R=1):
        mid, gauss, _ = self.spec
        phi = np.stack([np.ascontiguousarray(self.engine.get_draws(j)) for j in range(self.K)])
        return _newgroup.predict_new_group_host(mid, self.D, gauss, phi, Xn, gidx, labels, y, seed, t0, R)

    def loo(self, with_n=False):
        mid, gauss, sg = self.spec
        out = np.zeros((int(self.k_lim[self.K]), _loo.LO_COUNT))
        S = 0
        for j in range(self.K):
            lo, hi = int(self.k_lim[j]), int(self.k_lim[j + 1])
            theta = self.engine.get_draws(j, all_params=True)
            S = theta.shape[0]
            out[lo:hi] = _loo.loo_host(mid, self.D, int(self.site_ng[j]), gauss, theta, self.X[lo:hi],
                                       None if sg else self.j_ind[lo:hi] - 1, self.y[lo:hi])
        return (out, S) if with_n else out

    def replicated_checks(self, seed=0, row0=0, with_n=False, with_draws=False):
        mid, gauss, sg = self.spec
        thetas = [self.engine.get_draws(j, all_params=True) for j in range(self.K)]
        groups, sites, draws = _ppc.ppc_host(mid, self.D, self.site_ng, gauss, thetas, self.X,
                                             None if sg else self.j_ind - 1, self.y, self.k_lim, seed, row0)
        return (groups, sites) + ((draws,) if with_draws else ()) + ((thetas[-1].shape[0],) if with_n else ())

    def _diagnose(self, record_of, width, with_n):
        """(K, P, width) records of `record_of(theta, chains)`, NaN behind a site's own coordinates, and the used draws."""
        eng, chains = self.engine, self.chains
        pg = (eng.P - eng.d) // int(self.site_ng.max())          # coordinates per group behind phi
        loc = np.full((self.K, eng.P, width), np.nan)
        for j in range(self.K):
            Pk = eng.d + int(self.site_ng[j]) * pg
            theta = np.ascontiguousarray(eng.get_draws(j, all_params=True))
            loc[j, :Pk] = record_of(theta[:, :Pk], chains)
        return (loc, 2 * chains * ((theta.shape[0] // chains) // 2)) if with_n else loc

    def draw_diagnostics(self, with_n=False):
        return self._diagnose(_diagnostics.diagnostics_host, _diagnostics.DG_COUNT, with_n)

    def draw_rank_diagnostics(self, with_n=False):
        return self._diagnose(_diagnostics.rank_diagnostics_host, _diagnostics.RD_COUNT, with_n)


class Queries(object):
    """Answers each of QUERIES, CHECKS and INTERVALS, at every call, from `host.engine` (the engine at that time) where it has a method of
    that name and from `host` (a HostDraws over the same engine) where it has not: per method, since tests subclass both
    kinds of engine."""

    def __init__(self, host):
        self.host = host

    def __getattr__(self, name):
        if name not in QUERIES and name not in CHECKS and name not in INTERVALS:
            raise AttributeError(name)
        engine = self.host.engine
        return getattr(engine if hasattr(engine, name) else self.host, name)


# ---- per-site records of ALL sites on every rank

def gather_site_records(comm, K, local, widths, fill, head=None):
    """The flat records of all K sites from this rank's: `local` holds one 1-d record per local site, `widths` (K) the
    length of every site's (a local record may be longer than its width, up to the widest site's, where it holds `fill`
    behind its width: the device's diagnostics records are).  One column per site, padded with `fill` to the widest
    site, is gathered like the site arrays (`comm.allgather_sites`).  head: a number of this rank that travels in front of each of its records.  Returns
    (records (K, max(widths)), heads (K), None without `head`): site k's record is `records[k, :widths[k]]`, behind it
    lies `fill` and nothing else."""
    h = 0 if head is None else 1
    rec = np.full((h + int(max(widths)), len(local)), fill, dtype=np.float64, order='F')
    if h:
        rec[0, :] = head
    for j, flat in enumerate(local):
        rec[h:h + flat.size, j] = flat
    full = comm.allgather_sites(rec, K)
    return np.ascontiguousarray(full[h:, :].T), full[0, :] if h else None


def named_shapes(spec, D, site_ng, names):
    """Per site, the shape of every name's record at that site (site_params.named_shape)."""
    mid, gauss, sg = spec
    return [[_site_params.named_shape(mid, D, int(ng), gauss, sg, name) for name in names] for ng in site_ng]


def cut_named(rows, names, shapes):
    """rows (R, the elements of `names` side by side) -> {name: (R,) + the name's shape}."""
    out, at = {}, 0
    for name, sh in zip(names, shapes):
        size = int(np.prod(sh, dtype=np.int64))
        out[name] = rows[:, at:at + size].reshape((rows.shape[0],) + tuple(sh))
        at += size
    return out


def gather_named_records(comm, names, shapes, local, R, head=None):
    """gather_site_records for records of named parameters: `local` holds one {name: (R,) + the per-site shape} per local
    site, `shapes` named_shapes of all sites; returns one such dict per site, and the heads.  A site's record is its R rows
    of the site's elements side by side, flattened."""
    widths = [R * sum(int(np.prod(sh, dtype=np.int64)) for sh in row) for row in shapes]
    flat = [np.concatenate([d[name].reshape(R, -1) for name in names], axis=1).ravel() for d in local]
    recs, heads = gather_site_records(comm, len(shapes), flat, widths, 0.0, head)
    return [cut_named(rec[:w].reshape(R, w // R), names, shs) for rec, w, shs in zip(recs, widths, shapes)], heads


def gather_named_moments(comm, names, sites, n, means, m2s):
    """ns (K) and the lists of {name: mean}, {name: M2} of ALL sites from this rank's `named_moments`.  The record of a
    site is [n | means | M2s]: two rows behind the draws per site.  sites: (spec, D, site_ng) of all sites, as
    named_shapes takes them."""
    if comm.world == 1:
        return np.full(len(means), n, dtype=np.int64), means, m2s
    local = [dict((name, np.stack([np.asarray(m[name]), np.asarray(v[name])])) for name in names)
             for m, v in zip(means, m2s)]
    both, ns = gather_named_records(comm, names, named_shapes(*sites, names), local, 2, head=n)
    return (np.rint(ns).astype(np.int64), [dict((name, d[name][0]) for name in names) for d in both],
            [dict((name, d[name][1]) for name in names) for d in both])


def mix_moments(ns, ms, vs, params, smap, param_shapes):
    """(means, variances) of `params` from the sites' records (mix_pred.combine_moments per parameter)."""
    mean, var = [], []
    for ip, par in enumerate(params):
        m, v = _mix_pred.combine_moments(
            ns, [rec[par] for rec in ms], [rec[par] for rec in vs],
            smap[ip] if smap is not None else None, param_shapes[ip] if param_shapes is not None else None)
        mean.append(m)
        var.append(v)
    return mean, var


# ---- mix_quantiles

def pooled_shapes(spec, D, site_ng, names):
    """The shape of every name, which all sites have to hold alike to be pooled."""
    mid, gauss, sg = spec
    shapes = []
    for par in names:
        every = set(_site_params.named_shape(mid, D, int(ng), gauss, sg, par) for ng in site_ng)
        if len(every) != 1:
            raise ValueError("Without `smap` every site has to hold the whole parameter; the sites' records of "
                             "{!r} have the shapes {}".format(par, sorted(every)))
        shapes.append(every.pop())
    return shapes


def pooled_order_stats(queries, comm, names, shapes, ranks):
    """{name: (len(ranks),) + shape}: order statistics of the pool of ALL sites' draws of parameters every site holds,
    selected by counting over all ranks (quantiles.select_pooled)."""
    T = len(ranks)
    values, _, _ = _quantiles.select_pooled(lambda shift, prefix: queries.pooled_count_pass(names, shift, prefix, T),
                                            comm.allreduce_sum, ranks)
    return cut_named(np.ascontiguousarray(values.T), names, shapes)


def site_order_stats(queries, comm, names, sites, ranks):
    """Per-site order statistics of ALL sites on every rank: a list of {name: (len(ranks),) + per-site shape}.  Every
    rank selects its own sites'; with several ranks the records are gathered.  sites: as gather_named_moments takes it."""
    local = queries.named_order_stats(names, ranks)
    if comm.world == 1:
        return local
    return gather_named_records(comm, names, named_shapes(*sites, names), local, len(ranks))[0]


def place_site_quantiles(par, stats, ranks, plan, mp, shape):
    """(len(plan),) + shape: every site's own quantiles of `par` (stats: its order statistics per site) at the site's
    index `mp[k]` of the global parameter."""
    K = len(stats)
    if len(mp) != K:
        raise ValueError("Arg. `smap` of {!r} needs one index per site ({}), it has {}".format(par, K, len(mp)))
    filled = np.zeros(shape, dtype=np.int64)
    shape = filled.shape
    q = np.full((len(plan),) + shape, np.nan)
    for k in range(K):
        qk = _quantiles.interpolate(stats[k][par], ranks, plan)
        if qk.shape[1:] != np.shape(filled[mp[k]]):
            raise ValueError("The record of site {} has shape {}, its map addresses {} of the parameter {}"
                             .format(k, qk.shape[1:], np.shape(filled[mp[k]]), shape))
        filled[mp[k]] += 1
        for ir in range(len(plan)):
            q[ir][mp[k]] = qk[ir]
    if np.any(filled == 0):
        raise ValueError("Arg. `smap` does not fill the parameter {!r}".format(par))
    if np.any(filled > 1):
        raise ValueError("Arg. `smap` lets several sites fill one index of {!r}: the quantile of a pool of "
                         "sites is not a function of the sites' quantiles".format(par))
    return q


# ---- predict, predict_new_group, loo

def new_rows(X_new, D):
    """`X_new` of predict / predict_new_group as float64 (n, D)."""
    X_new = np.asarray(X_new, dtype=np.float64)
    if X_new.ndim != 2 or X_new.shape[1] != D:
        raise ValueError("Argument `X_new` should be two dimensional with {} columns".format(D))
    return X_new


def new_responses(y_new, n, gauss, finite, model_name):
    """`y_new` of predict / predict_new_group as contiguous float64 (n,), or None.  The Bernoulli models take 0 or
    1; the Gaussian ones anything, or with `finite` (a new group's joint term adds its rows' terms up) finite
    values only."""
    if y_new is None:
        return None
    ys = np.ascontiguousarray(y_new, dtype=np.float64)
    if ys.shape != (n,):
        raise ValueError("The shapes of `y_new` and `X_new` does not match")
    if gauss and not finite:
        return ys
    bad = np.nonzero(~np.isfinite(ys) if gauss else (ys != 0) & (ys != 1))[0]
    if bad.size:
        raise ValueError("`y_new` of row {}: {}; site model {!r} takes {}".format(
            int(bad[0]), ys[bad[0]], model_name, "finite responses" if gauss else "responses 0 or 1"))
    return ys


def predictive_result(rec, has_y, n, **more):
    """The result of predict / predict_new_group from the records `rec` (rows, 4) over n draws or pool members."""
    return dict(mean=rec[:, _site_params.PR_MEAN].copy(), f_mean=rec[:, _site_params.PR_F_MEAN].copy(),
                f_var=rec[:, _site_params.PR_F_M2] / (n - 1),
                lpd=rec[:, _site_params.PR_LPD].copy() if has_y else None, **more, n=n)


def plan_rows(n, K, site_sizes, site_ind, j_ind, site_ng, single_group, model_name):
    """predict's n new rows sorted by site: (rows, lim, group) -- the caller's row of every sorted row, the K + 1 row limits
    of the sites, and the 0-based group within its site of every sorted row (None for a single-group model).  The site of
    every row comes as `site_sizes` if given, as `site_ind` otherwise; `j_ind`, `site_ng` (K): the 1-based group of every
    row and the groups of every site."""
    order = None
    if site_sizes is not None:
        cnt = np.asarray(site_sizes, dtype=np.int64)
        if cnt.shape != (K,) or np.any(cnt < 0) or cnt.sum() != n:
            raise ValueError("`site_sizes`: {} non-negative counts that add up to the rows of `X_new`".format(K))
    else:
        site_ind = np.asarray(site_ind)
        if site_ind.shape != (n,) or not np.issubdtype(site_ind.dtype, np.integer) \
                or (n and (site_ind.min() < 0 or site_ind.max() >= K)):
            raise ValueError("`site_ind`: one site index in [0, {}) per row of `X_new`".format(K))
        order = np.argsort(site_ind, kind='mergesort')       # stable: rows keep their order inside a site
        cnt = np.bincount(site_ind, minlength=K).astype(np.int64)
    lim = np.concatenate(([0], np.cumsum(cnt)))
    rows = np.arange(n) if order is None else order
    group = None
    if single_group:
        if j_ind is not None:
            raise ValueError("site model {!r} holds one group per site: it takes no `j_ind`".format(model_name))
    else:
        if j_ind is None:
            raise ValueError("site model {!r} holds several groups per site: give the 1-based group of every "
                             "new row within its site as `j_ind`".format(model_name))
        j_ind = np.asarray(j_ind)
        if j_ind.shape != (n,) or not np.issubdtype(j_ind.dtype, np.integer):
            raise ValueError("`j_ind`: one integer per row of `X_new`")
        group = (j_ind[rows] - 1).astype(np.int32)
        bad = np.nonzero((group < 0) | (group >= np.repeat(site_ng, cnt)))[0]
        if bad.size:
            i = int(bad[0])
            k = int(np.searchsorted(lim, i, side='right') - 1)
            raise ValueError("`j_ind` of row {}: group {} outside 1..{} of site {}"
                             .format(int(rows[i]), int(group[i]) + 1, int(site_ng[k]), k))
    return rows, lim, group


def sum_predict_rows(comm, local, lo, hi, n, has_y):
    """predict's (n, 4) records on every rank from the rows [lo, hi) of this rank's sites: one sum over the ranks."""
    rec = np.zeros((n, _site_params.PR_COUNT))
    rec[lo:hi] = local
    if not has_y:
        rec[:, _site_params.PR_LPD] = 0.0                    # (NaN without responses: nothing to add up)
    return comm.allreduce_sum(rec) if n else rec


def merge_new_group(comm, rows, glpd, N, has_y):
    """predict_new_group's (rows, glpd, N) over the pool of all ranks' draws from this rank's: every rank's record in its
    own slot, one sum, the pools merged in rank order (newgroup.merge)."""
    world, C = comm.world, _site_params.PR_COUNT
    if world == 1:
        return rows, glpd, N
    n = rows.shape[0]
    width = n * C + len(glpd) + 1
    rec = np.zeros((world, width))
    mine = np.concatenate((rows.reshape(-1), glpd, [float(N)]))
    rec[comm.rank] = mine if has_y else np.where(np.isnan(mine), 0.0, mine)
    rec = np.asarray(comm.allreduce_sum(rec.reshape(-1))).reshape(world, width)
    return _newgroup.merge([(rec[r, :n * C].reshape(n, C), rec[r, n * C:-1], int(round(rec[r, -1])))
                            for r in range(world)])


def sum_loo_rows(comm, loc, lo, hi, N):
    """loo's (N, 6) records on every rank from the rows [lo, hi) of this rank's sites.  A sum carries neither NaN (a row
    with a non-finite log-likelihood) nor +inf (KHAT of a row that was not smoothed) next to the other ranks' zeros: they
    travel as a code beside the records."""
    if comm.world == 1:
        return loc
    C = _loo.LO_COUNT
    both = np.zeros((N, 2 * C))
    both[lo:hi, :C] = np.where(np.isfinite(loc), loc, 0.0)
    both[lo:hi, C:] = np.where(np.isnan(loc), 1.0, np.where(loc == np.inf, 2.0, np.where(loc == -np.inf, 3.0, 0.0)))
    both = comm.allreduce_sum(both)
    rec, code = both[:, :C], both[:, C:]
    return np.where(code == 1.0, np.nan, np.where(code == 2.0, np.inf, np.where(code == 3.0, -np.inf, rec)))


def sum_order_rows(comm, loc, lo, hi, n):
    """predict_quantiles' (n, T) order statistics on every rank from the rows [lo, hi) of this rank's sites: every rank's
    rows in a zero-filled (n, T) array, one sum over the ranks.  NaN (a row with a NaN value) and +-inf (ordinary
    values of an order statistic) travel as a code beside the values, as in `sum_loo_rows`; so does -0.0, whose sign a
    sum with the other ranks' zeros would drop: every value arrives with the bits it had (a NaN as the default NaN)."""
    if comm.world == 1:
        return loc
    T = loc.shape[1]
    both = np.zeros((n, 2 * T))
    both[lo:hi, :T] = np.where(np.isfinite(loc), loc, 0.0)
    both[lo:hi, T:] = np.where(np.isnan(loc), 1.0, np.where(loc == np.inf, 2.0, np.where(loc == -np.inf, 3.0, np.where(
        (loc == 0.0) & np.signbit(loc), 4.0, 0.0))))
    both = comm.allreduce_sum(both) if n else both
    rec, code = both[:, :T], both[:, T:]
    return np.where(code == 1.0, np.nan, np.where(code == 2.0, np.inf, np.where(code == 3.0, -np.inf, np.where(
        code == 4.0, -0.0, rec))))


# ---- ppc

def gather_checks(comm, site_ng, k_lo, groups, sites, n):
    """(groups (G, 8), sites (K, 8), ns (K)) of ALL sites from this rank's `replicated_checks` records, those of the
    sites k_lo, k_lo + 1, ...  A site's flat record is its site record followed by its groups' records: widths differ with
    `site_ng` (K, all sites), the fill is NaN; the draws per site travel as the head."""
    C = _ppc.PC_COUNT
    site_ng = np.asarray(site_ng, dtype=np.int64)
    K = site_ng.shape[0]
    if comm.world == 1:
        return groups, sites, np.full(K, n, dtype=np.int64)
    flat, at = [], 0
    for j in range(sites.shape[0]):
        ng = int(site_ng[k_lo + j])
        flat.append(np.concatenate((sites[j], groups[at:at + ng].ravel())))
        at += ng
    recs, heads = gather_site_records(comm, K, flat, C * (1 + site_ng), np.nan, n)
    all_groups = np.concatenate([recs[k, C:C * (1 + int(site_ng[k]))].reshape(int(site_ng[k]), C) for k in range(K)])
    return all_groups, np.ascontiguousarray(recs[:, :C]), np.rint(heads).astype(np.int64)


# ---- log_evidence

def site_evidence_records(host, seed, site0):
    """(records (K_local, EV_COUNT), ms) of this rank's sites from the draws of the last sampling call: the engine's
    `site_evidence` where it has one, else `evidence.site_evidence_host` over its `get_draws` and `get_cavity` (host: the
    HostDraws of the Master)."""
    engine = host.engine
    if hasattr(engine, 'site_evidence'):
        out, _, ms = engine.site_evidence(seed=seed, site0=site0)
        return out, ms
    mid, gauss, sg = host.spec
    out = np.empty((host.K, _evidence.EV_COUNT))
    for j in range(host.K):
        lo, hi = int(host.k_lim[j]), int(host.k_lim[j + 1])
        P = _evidence.site_dims(mid, host.D, gauss, int(host.site_ng[j]))[1]
        theta = np.ascontiguousarray(engine.get_draws(j, all_params=True))[:, :P]
        Om, mu = engine.get_cavity(j)
        out[j] = _evidence.site_evidence_host(mid, host.D, gauss, host.X[lo:hi], host.y[lo:hi],
                                              None if sg else host.j_ind[lo:hi] - 1, mu, Om, theta, host.chains, seed,
                                              site0 + j)[0]
    return out, 0.0


def gather_evidence(comm, K, local):
    """(K, width) records of ALL sites from this rank's `local` (K_local, width)."""
    if comm.world == 1:
        return local
    return gather_site_records(comm, K, list(local), np.full(K, local.shape[1], dtype=np.int64), np.nan)[0]


# ---- diagnostics

def gather_diagnostics(comm, site_P, loc, head=None):
    """(K, Pmax, width) diagnostics records of ALL sites from this rank's `loc` (K_local, P, width), NaN behind a site's
    own `site_P[k]` coordinates, and the heads (K) where `head` (the used draws) is given."""
    K, width = len(site_P), loc.shape[2]
    recs, heads = gather_site_records(comm, K, [rec.ravel() for rec in loc], site_P * width, np.nan, head)
    return recs.reshape(K, int(site_P.max()), width), heads
