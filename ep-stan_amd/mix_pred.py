"""Combination of per-site moments into one parameter's mean and variance (`Master.mix_pred`).

Restates the combination step of /root/reference/epstan/method.py:1366-1472 as a pure function of
per-site records: draws per site `ns[k]`, site means `ms[k]` and CENTRED sums of squares
`vs[k] = sum_s (x_s - ms[k])^2`, each in the site's own shape.  Where the records come from -- the
device kernel `k_named_moments` or `site_params.named_moments_host` -- is the caller's business.

(The reference forms its first worker's sum of squares in the `smap is None` branch as
`sum x^2 - n mean^2`, method.py:1382; the centred form used here for every site agrees to rounding.)
"""

import numpy as np


def combine_moments(ns, ms, vs, smap=None, param_shape=None):
    """(mean, var) of one parameter from the sites' records.

    smap None: every site holds the whole parameter; the sites' draws are pooled,
        var = (sum_k vs_k + sum_k n_k (m_k - m)^2) / (n - 1).
    smap[k]: NumPy index of site k's elements in the parameter of shape `param_shape`.
      * every index filled by one site: that site's own mean and vs / (n_k - 1);
      * some index filled by several sites: the reference pools them per index and then, when ANY
        index has a single contribution, assigns every site's own values to ALL of the site's
        indexes in site order (method.py:1464-1469) -- so a shared index ends with the moments of
        the LAST site that maps to it, and the pooled value survives only when no index is
        single.  Reproduced as it behaves: the golden vectors are the reference's results.
    A map that leaves an index of the parameter without a contribution raises ValueError."""
    ns = np.asarray(ns, dtype=np.int64)
    K = ns.shape[0]
    if len(ms) != K or len(vs) != K:
        raise ValueError("one record per site is needed")
    if smap is None:
        shapes = set(np.shape(m) for m in ms) | set(np.shape(v) for v in vs)
        if len(shapes) != 1:
            raise ValueError("Without `smap` every site has to hold the whole parameter; the sites' records have "
                             "the shapes {}".format(sorted(shapes)))
        ms = np.stack([np.asarray(m, dtype=np.float64) for m in ms])
        vs = np.stack([np.asarray(v, dtype=np.float64) for v in vs])
        w = ns.reshape((K,) + (1,) * (ms.ndim - 1)).astype(np.float64)
        n = ns.sum()
        mean = np.sum(w * ms, axis=0) / n
        var = np.sum(vs + w * np.square(ms - mean), axis=0) / (n - 1)
        return mean, var
    if param_shape is None:
        raise ValueError("Arg. `param_shapes` has to be given with `smap`")
    count = np.zeros(param_shape)
    for k in range(K):
        if np.shape(ms[k]) != np.shape(count[smap[k]]) or np.shape(vs[k]) != np.shape(ms[k]):
            raise ValueError("The record of site {} has shape {}, its map addresses {} of the parameter {}"
                             .format(k, np.shape(ms[k]), np.shape(count[smap[k]]), tuple(param_shape)))
        count[smap[k]] += 1
    if np.count_nonzero(count) != count.size:
        raise ValueError("Arg. `smap` does not fill the parameter")
    single = count == 1
    mean = np.zeros(param_shape)
    var = np.zeros(param_shape)
    if not np.all(single):
        nc = np.zeros(param_shape, dtype=np.int64)
        for k in range(K):
            nc[smap[k]] += ns[k]
            mean[smap[k]] += ns[k] * np.asarray(ms[k])
        mean /= nc
        for k in range(K):
            var[smap[k]] += np.asarray(vs[k]) + ns[k] * np.square(np.asarray(ms[k]) - mean[smap[k]])
        var /= nc - 1
    if np.any(single):
        for k in range(K):
            mean[smap[k]] = ms[k]
            var[smap[k]] = np.asarray(vs[k]) / (ns[k] - 1)
    return mean, var
