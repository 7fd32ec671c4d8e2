"""Posterior predictive of a group that was NOT in the data, restated in NumPy: the definition at
`epx_predict_new_group` (include/epx.h), which the device kernels k_newgroup / k_newgroup_merge / k_newgroup_latents
(csrc/newgroup.inc) follow too.  The expectation of their tests, and `Master.predict_new_group`'s route on an engine
without `predict_new_group`.

The new group's own latents eta, etb are drawn from the model's prior (standard normal for m1..m4, standard Laplace for
m5) by the counter-based Philox4x32-10 stream of the samplers (csrc/epx_device.h, oracle/nuts_oracle.c), kind
K_NEWGROUP: a latent depends on (seed, label, pooled draw index t, replicate r, element e) only.
"""

import numpy as np

from . import site_params as _site_params

K_NEWGROUP = 6                                           # the stream's kind, next to K_INIT .. K_SSMOM = 5 (csrc/epx_kernels.h)
R_MAX = 1024
_M32 = np.uint64(0xFFFFFFFF)


def make_key(seed, chain):
    """(k0, k1) of the stream of `chain` under `seed` (a 64-bit unsigned integer): csrc/epx_device.h make_key."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, ((seed >> 32) ^ (0x85EBCA6B * ((int(chain) + 1) & 0xFFFFFFFF))) & 0xFFFFFFFF


def philox4x32(key, c0, c1, c2, c3):
    """Philox4x32-10 of the counters (arrays of 32-bit values, broadcast against each other) under `key`: four uint64
    arrays holding 32-bit words."""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & _M32 for c in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                        # 32 x 32 bits: no overflow of 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def u01(hi, lo):
    """Uniform on the OPEN interval: (v + 1/2) 2^-53 of the 53-bit integer v = hi : lo >> 11."""
    v = (hi << np.uint64(21)) | (lo >> np.uint64(11))
    return (v.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def rng_u2(key, t, kind, a, b):
    """The two uniforms of counter (t, kind, a, b): csrc/epx_device.h rng_u2, bit for bit."""
    o = philox4x32(key, t, kind, a, b)
    return u01(o[0], o[1]), u01(o[2], o[3])


def n_latents(mid, D):
    """E: eta alone for m1 (its beta is part of phi), eta and etb (D) for m2..m5."""
    return 1 if mid == 0 else 1 + D


def latents_host(mid, D, seed, label, t, R):
    """z (len(t), R, E) of new group `label` at the pooled draws t and replicates 0..R: element 0 is eta, 1 + j is etb_j.
    m1..m4: the Box-Muller pair of (u1, u2) = rng_u2(key, t, K_NEWGROUP, e >> 1, r), cosine for even e; m5: the inverse
    Laplace distribution function of u1 (even e) or u2 (odd e)."""
    t = np.asarray(t, dtype=np.uint64).reshape(-1)
    E = n_latents(mid, D)
    key = make_key(seed, label)
    z = np.empty((t.shape[0], R, E))
    r = np.arange(R, dtype=np.uint64)[None, :]
    for p in range((E + 1) // 2):
        u1, u2 = rng_u2(key, t[:, None], K_NEWGROUP, p, r)
        if mid == 4:
            pair = [np.copysign(-np.log1p(-2.0 * np.abs(u - 0.5)), u - 0.5) for u in (u1, u2)]
        else:
            rad, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586476925286766559 * u2
            pair = [rad * np.cos(ang), rad * np.sin(ang)]
        for h in range(2):
            if 2 * p + h < E:
                z[:, :, 2 * p + h] = pair[h]
    return z


def coefficients(mid, D, gauss, phi, z):
    """alpha (T, R) and beta (T, R or 1, D) of the new group from phi (T, d) and its latents z (T, R, E): the
    `transformed parameters` of the Stan programs with eta := z_0, etb_j := z_{1+j}."""
    b = phi[:, (1 if gauss else 0):]
    eta, etb = z[:, :, 0], z[:, :, 1:]
    if mid == 0:                                         # phi = [log sigma_a, beta]
        return eta * np.exp(b[:, 0])[:, None], b[:, None, 1:1 + D]
    if mid == 1:                                         # phi = [log sigma_a, log sigma_b]
        return eta * np.exp(b[:, 0])[:, None], etb * np.exp(b[:, 1])[:, None, None]
    if mid == 2:                                         # phi = [log sigma_a, log sigma_b (D)]
        return eta * np.exp(b[:, 0])[:, None], etb * np.exp(b[:, 1:1 + D])[:, None, :]
    # phi = [mu_a, log sigma_a, mu_b (D), log sigma_b (D)]
    return (b[:, 0][:, None] + eta * np.exp(b[:, 1])[:, None],
            b[:, None, 2:2 + D] + etb * np.exp(b[:, 2 + D:2 + 2 * D])[:, None, :])


def _log_mean_exp(ll):
    top = ll.max(axis=0)
    return top + np.log(np.exp(ll - top).mean(axis=0))


def predict_new_group_host(mid, D, gauss, phi, Xn, gidx, labels, y, seed, t0, R):
    """(rows (n, 4), glpd (G,), N) of the new rows Xn (n, D) from the pool of draws phi (count, S, d): row i belongs to
    new group gidx[i] (dense, 0..G-1; None: all 0) whose stream label is labels[gidx[i]]; t0: pooled index of the first
    draw.  Columns of `rows` as site_params.predict_host, over the N = count S R pool members; glpd: the joint log
    predictive density of every group's responses (0 for a group without rows, NaN without y)."""
    phi = np.asarray(phi, dtype=np.float64)
    count, S = phi.shape[:2]
    T, N = count * S, count * S * R
    phi = phi.reshape(T, -1)
    Xn = np.asarray(Xn, dtype=np.float64).reshape(-1, D)
    n = Xn.shape[0]
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    G = labels.shape[0]
    gidx = np.zeros(n, dtype=np.int64) if gidx is None else np.asarray(gidx, dtype=np.int64)
    if gidx.shape != (n,) or (n and (gidx.min() < 0 or gidx.max() >= G)):
        raise ValueError("gidx: one 0-based index below {} per new row".format(G))
    if np.any(labels < 0) or np.any(labels >= 2 ** 31):
        raise ValueError("labels: integers in [0, 2^31)")
    if not 1 <= R <= R_MAX:
        raise ValueError("R must be in 1..{}".format(R_MAX))
    if t0 < 0 or t0 + T > 2 ** 32:
        raise ValueError("pooled draws [{}, {}) outside [0, 2^32)".format(t0, t0 + T))
    y = None if y is None else np.asarray(y, dtype=np.float64)
    rows = np.full((n, _site_params.PR_COUNT), np.nan)
    glpd = np.full(G, np.nan) if y is None else np.zeros(G)
    t = t0 + np.arange(T, dtype=np.int64)
    ls = np.repeat(phi[:, :1], R, axis=0)                # (N, 1): log sigma of the Gaussian family, per pool member
    for g in np.unique(gidx):
        at = np.nonzero(gidx == g)[0]
        z = latents_host(mid, D, seed, int(labels[g]), t, R)
        alpha, beta = coefficients(mid, D, gauss, phi, z)
        f = (alpha[:, :, None] + np.matmul(beta, Xn[at].T)).reshape(N, at.shape[0])      # member n = (t, r)
        fm = f.mean(axis=0)
        rows[at, _site_params.PR_F_MEAN] = fm
        rows[at, _site_params.PR_F_M2] = np.square(f - fm).sum(axis=0)
        if gauss:
            rows[at, _site_params.PR_MEAN] = fm
        else:
            e = np.exp(-np.abs(f))
            rows[at, _site_params.PR_MEAN] = np.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e)).mean(axis=0)
        if y is not None:
            ll = _site_params.loglik_of(gauss, ls, f, y[at])
            rows[at, _site_params.PR_LPD] = _log_mean_exp(ll)
            glpd[g] = _log_mean_exp(ll.sum(axis=1))
    return rows, glpd, N


def _merge_lme(a, Na, b, Nb):
    """log-mean-exp of the union of two pools from theirs: logaddexp(a + log Na, b + log Nb) - log N, written about the
    larger of the two (equal inputs come back as they are)."""
    with np.errstate(invalid='ignore', divide='ignore'):
        top = np.maximum(a, b)
        return top + np.log((Na * np.exp(a - top) + Nb * np.exp(b - top)) / (Na + Nb))


def merge(parts):
    """(rows, glpd, N) of the union of disjoint pools from their results, taken in the order given: the means by
    weights, M2 = M2_a + M2_b + (fmean_a - fmean_b)^2 N_a N_b / N, LPD and GLPD as log-mean-exps."""
    PR = _site_params
    rows, glpd, Na = np.array(parts[0][0], dtype=np.float64), np.array(parts[0][1], dtype=np.float64), int(parts[0][2])
    for rb, gb, Nb in parts[1:]:
        rb, gb, Nb = np.asarray(rb, dtype=np.float64), np.asarray(gb, dtype=np.float64), int(Nb)
        N = Na + Nb
        out = np.empty_like(rows)
        dlt = rows[:, PR.PR_F_MEAN] - rb[:, PR.PR_F_MEAN]
        out[:, PR.PR_F_M2] = rows[:, PR.PR_F_M2] + rb[:, PR.PR_F_M2] + dlt * dlt * (float(Na) * Nb / N)
        for col in (PR.PR_MEAN, PR.PR_F_MEAN):
            out[:, col] = (Na * rows[:, col] + Nb * rb[:, col]) / N
        out[:, PR.PR_LPD] = _merge_lme(rows[:, PR.PR_LPD], Na, rb[:, PR.PR_LPD], Nb)
        glpd = _merge_lme(glpd, Na, gb, Nb)
        rows, Na = out, N
    return rows, glpd, Na
