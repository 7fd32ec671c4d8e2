"""Posterior quantiles of named parameters from order statistics across draws (`Master.mix_quantiles`), in plain NumPy.

The definition is stated in include/epx.h ("Posterior quantiles"): the total order of doubles by their key, the type-7
quantile, NaN for an element with a NaN draw.  The device delivers ORDER STATISTICS -- per site from k_site_order_stats,
over the pool of all sites' draws by eight counting passes of k_pooled_count (csrc/quantiles.inc) -- and the host
interpolates.  This module holds the host's share (`rank_plan`, `interpolate`, `select_pooled`) and the host restatement
of the device's (`order_stats`, `site_order_stats_host`, `site_quantiles_host`, `count_pass_host`): the expectation of the
kernels' tests and `Master.mix_quantiles`' route on an engine without the device methods."""

import numpy as np

from . import site_params

MAX_RANKS = 32                 # EPX_QT_MAX_RANKS (csrc/epx_kernels.h): ranks / targets of one call
_SIGN = np.uint64(1 << 63)
_ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def key_of(x):
    """uint64 keys of doubles (csrc/order_key.h): the IEEE-754 bits, all flipped when the sign bit is set, else the sign
    bit set: -inf < ... < -0.0 < +0.0 < ... < +inf as unsigned integers."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where((b & _SIGN) != 0, b ^ _ALL, b | _SIGN)


def value_of(k):
    """The doubles behind keys: the inverse of `key_of`, bit for bit."""
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where((k & _SIGN) != 0, k ^ _SIGN, k ^ _ALL).view(np.float64)


def rank_plan(n, probs):
    """(ranks, plan) for the quantiles at `probs` of n draws: plan[j] = (i, g) with h = p (n - 1), i = min(floor(h), n - 2),
    g = h - i (n = 1: (0, 0.0)); ranks = the distinct i and i + 1 ascending (int64), what has to be selected.  A p outside
    [0, 1] or NaN, an n < 1 and more than MAX_RANKS ranks are ValueErrors."""
    n = int(n)
    if n < 1:
        raise ValueError("quantiles need at least one draw (n = {})".format(n))
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    if probs.ndim != 1 or probs.size < 1 or not np.all((probs >= 0.0) & (probs <= 1.0)):       # (NaN fails both)
        raise ValueError("probs: probabilities in [0, 1] (got {})".format(probs))
    plan, need = [], set()
    for p in probs:
        if n == 1:
            i, g = 0, 0.0
            need.add(0)
        else:
            h = float(p) * (n - 1)
            i = min(int(np.floor(h)), n - 2)
            g = h - i
            need.update((i, i + 1))
        plan.append((i, g))
    ranks = np.array(sorted(need), dtype=np.int64)
    if ranks.size > MAX_RANKS:
        raise ValueError("{} probabilities need {} order statistics, at most {} in one call".format(
            probs.size, ranks.size, MAX_RANKS))
    return ranks, plan


def interpolate(stats, ranks, plan):
    """Quantiles (len(plan),) + shape from the order statistics stats (len(ranks),) + shape of `rank_plan`'s ranks:
    x_(i) + g (x_(i+1) - x_(i)) in exactly that form; one draw: x_(0)."""
    stats = np.asarray(stats, dtype=np.float64)
    ranks = np.asarray(ranks, dtype=np.int64)
    if stats.shape[0] != ranks.shape[0]:
        raise ValueError("one order statistic per rank is needed")
    out = np.empty((len(plan),) + stats.shape[1:])
    with np.errstate(invalid='ignore', over='ignore'):
        for j, (i, g) in enumerate(plan):
            at = int(np.searchsorted(ranks, i))
            if ranks.size == 1:                              # n = 1
                out[j] = stats[at]
            else:
                out[j] = stats[at] + g * (stats[at + 1] - stats[at])
    return out


def order_stats(x, ranks):
    """x_(r) for r in ranks along axis 0 of x (n, ...): (len(ranks), ...), ordered by key; an element (column) with any
    NaN has NaN at every rank."""
    x = np.asarray(x, dtype=np.float64)
    ranks = np.asarray(ranks, dtype=np.int64)
    if ranks.size and (ranks.min() < 0 or ranks.max() >= x.shape[0]):
        raise ValueError("a rank outside [0, {})".format(x.shape[0]))
    flat = x.reshape(x.shape[0], -1)
    out = value_of(np.sort(key_of(flat), axis=0)[ranks])
    out[:, np.isnan(flat).any(axis=0)] = np.nan
    return out.reshape((ranks.size,) + x.shape[1:])


def site_order_stats_host(model_id, D, ng, gauss, single_group, theta, names, ranks):
    """{name: (len(ranks),) + per-site shape}: the order statistics of the named parameters of ONE site from its draws
    theta (S, P), formed by site_params.named_draws and sorted by key.  What k_site_order_stats computes."""
    draws = site_params.named_draws(model_id, D, ng, gauss, single_group, theta, names)
    return dict((name, order_stats(draws[name], ranks)) for name in names)


def site_quantiles_host(model_id, D, ng, gauss, single_group, theta, names, probs):
    """{name: (len(probs),) + per-site shape}: the quantiles of the named parameters of ONE site from its draws theta."""
    ranks, plan = rank_plan(np.asarray(theta).shape[0], probs)
    stats = site_order_stats_host(model_id, D, ng, gauss, single_group, theta, names, ranks)
    return dict((name, interpolate(stats[name], ranks, plan)) for name in names)


def count_pass_host(x, shift, prefix, n_targets):
    """One counting pass (epx_pooled_count_pass, include/epx.h) over the draws x (n, L) of L elements:
    (hist (L, n_targets, 256) int64, n_nan (L) int64, n).  hist[e, t, b] = the draws of element e whose key agrees with
    prefix[e, t] (uint64) in all bits above shift + 7 and whose byte at `shift` is b; at shift 56 every draw counts and
    prefix is not read.  NaN draws count by their keys and in n_nan besides."""
    x = np.asarray(x, dtype=np.float64)
    n, L = x.shape
    keys = key_of(x)
    byte = ((keys >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
    hist = np.zeros((L, n_targets, 256), dtype=np.int64)
    if shift < 56:
        prefix = np.asarray(prefix, dtype=np.uint64).reshape(L, n_targets)
    for e in range(L):
        for t in range(n_targets):
            sel = byte[:, e]
            if shift < 56:
                sel = sel[((keys[:, e] ^ prefix[e, t]) >> np.uint64(shift + 8)) == 0]
            hist[e, t] = np.bincount(sel, minlength=256)
    return hist, np.isnan(x).sum(axis=0).astype(np.int64), n


def select_pooled(count_pass, allreduce_sum, ranks):
    """Order statistics of a pool of draws that lies in several shards (workgroups, devices, ranks), selected by counting,
    most significant byte first: (values (L, len(ranks)) float64, n_nan (L) int64, n).

    count_pass(shift, prefix) -> (hist (L, T, 256), n_nan (L), n): this shard's counts for the (L, T) uint64 key prefixes
    (HipEngine.pooled_count_pass, count_pass_host); allreduce_sum(a): sums a float64 array over the shards in place and
    returns it (a communicator's; the identity for one shard).  Counts travel as float64, which is exact below 2^53
    draws.  Per (element, target) the cumulative counts are walked to the byte that holds the remaining rank, the prefix
    is extended by it and the rank reduced by the counts below; behind the pass at shift 0 the prefix is the key of
    x_(r).  ranks (T): 0-based, below the pool's n, the same for every element.  An element with NaN draws (n_nan > 0) has
    NaN at every rank."""
    ranks = np.asarray(ranks, dtype=np.int64).ravel()
    T = ranks.size
    if T < 1 or T > MAX_RANKS:
        raise ValueError("between 1 and {} ranks".format(MAX_RANKS))
    prefix = rem = n_nan = n = None
    for shift in range(56, -8, -8):
        hist, nn, nl = count_pass(shift, prefix)
        hist = np.asarray(hist)
        L = hist.shape[0]
        buf = np.concatenate([hist.reshape(-1).astype(np.float64), np.asarray(nn, dtype=np.float64).reshape(-1),
                              [float(nl)]])
        buf = np.rint(allreduce_sum(buf)).astype(np.int64)
        hist = buf[:L * T * 256].reshape(L, T, 256)
        if prefix is None:
            n_nan, n = buf[L * T * 256:-1].copy(), int(buf[-1])
            if ranks.min() < 0 or ranks.max() >= n:
                raise ValueError("a rank outside [0, {}), the draws of the pool".format(n))
            prefix = np.zeros((L, T), dtype=np.uint64)
            rem = np.broadcast_to(ranks, (L, T)).copy()
        cum = np.cumsum(hist, axis=2)
        b = (cum <= rem[:, :, None]).sum(axis=2)             # the first byte whose cumulative count exceeds the rank
        if b.max() > 255:
            raise RuntimeError("the counts of the pass at shift {} do not hold the ranks".format(shift))
        below = np.where(b > 0, np.take_along_axis(cum, np.maximum(b - 1, 0)[:, :, None], axis=2)[:, :, 0], 0)
        rem -= below
        prefix |= b.astype(np.uint64) << np.uint64(shift)
    values = value_of(prefix)
    values[n_nan > 0, :] = np.nan
    return values, n_nan, n
