"""The marginal likelihood of EP, restated in NumPy: the definition at `epx_site_evidence` (include/epx.h), which the
device kernels k_ev_fit / k_ev_bridge (csrc/evidence.hip) and k_ev_terms (csrc/evidence_terms.inc) follow too.  The
expectation of their tests.

Per site, `site_evidence_host` estimates log int exp(lq) -- lq the unnormalised log density the site's sampler draws
from -- by bridge sampling between the site's tilted draws and a Gaussian proposal fitted to the first half of every
chain.  `site_log_z` turns that into log Z_k against the normalised cavity and the normalised prior of the latents, and
`combine` adds the sites up into log Z_EP from the natural parameters of the approximation.

Everything works in the dtype it is given (float64, or np.longdouble for the tests' error scale); the proposal's normals
come from the samplers' Philox stream through `newgroup`'s twin, kind K_BRIDGE, always in float64 as on the device.
"""

import math

import numpy as np

from . import loo as _loo
from . import newgroup as _newgroup

# enum epx_evidence (include/epx.h): the columns of a site's record
EV_LOGZ, EV_LOGZ_IS, EV_ITERS, EV_RE2, EV_KHAT, EV_N1, EV_COUNT = 0, 1, 2, 3, 4, 5, 6
K_BRIDGE = 8                                             # the stream's kind, next to K_PPC = 7 (csrc/epx_kernels.h)
TOL, MAX_ITERS = 1e-10, 1000
D_MAX = 128                                              # EPX_PR_DMAX
_LDS_BYTES = 160 * 1024                                  # lds_capacity() (csrc/nuts_geometry.h)
_LOG_2PI = math.log(2.0 * math.pi)


def _log_2pi(dt):
    """log 2 pi in the scalar type dt."""
    return np.log(dt(8) * np.arctan(dt(1)))


# ---- sizes and refusals

def site_dims(mid, D, gauss, ng=1):
    """(d, P) of a site with ng groups: dphi and the sampled coordinates theta = [phi | eta (ng) | etb (ng x D)]."""
    d = (1 if gauss else 0) + {0: D + 1, 1: 2, 2: D + 1, 3: 2 * D + 2, 4: 2 * D + 2}[mid]
    return d, d + ng * (1 if mid == 0 else 1 + D)


def n_latents(mid, D, ng=1):
    """Latents lambda of a site: eta per group, and etb per group x D for m2..m5."""
    return ng * (1 if mid == 0 else 1 + D)


def split_sizes(S, chains):
    """(|F|, N1) of S draws in `chains` chains: F is the first floor(n / 2) draws of every chain, E the rest."""
    n = S // chains
    return (n // 2) * chains, S - (n // 2) * chains


def split(S, chains):
    """The draw indices (device order, chain-major) of F and of E."""
    n = S // chains
    i = np.arange(S).reshape(chains, n)
    return i[:, :n // 2].ravel(), i[:, n // 2:].ravel()


def _terms_doubles(P, KP):
    """evidence_terms_doubles (csrc/epx_kernels.h)."""
    return P * (P + 1) // 2 + 2 * P + 32 * (P | 1) + KP * 16 + 32 + 64 + 32


def max_coords(D):
    """evidence_max_coords (csrc/epx_kernels.h): most sampled coordinates whose packed factor and workspace fit the LDS."""
    KP = (1 + D + 3) // 4 * 4
    P = 1
    while _terms_doubles(P + 1, KP) * 8 <= _LDS_BYTES - 1024:
        P += 1
    return P


def check_sizes(S, chains, P, D):
    """The refusals of `epx_site_evidence` that are known from sizes alone, as ValueErrors that name the numbers."""
    if D > D_MAX:
        raise ValueError("D = {} columns, at most {}".format(D, D_MAX))
    if P > max_coords(D):
        raise ValueError("P = {} sampled coordinates, at most {} at D = {} (the packed factor of the proposal and the "
                         "slab's workspace are kept in LDS)".format(P, max_coords(D), D))
    if chains < 1 or S < 1 or S % chains != 0:
        raise ValueError("S = {} draws are no multiple of chains = {}".format(S, chains))
    nF = split_sizes(S, chains)[0]
    if nF < 2 * P:
        raise ValueError("the fit set holds {} draws (the first {} of each of {} chains), the proposal of P = {} "
                         "coordinates needs at least {}".format(nF, S // chains // 2, chains, P, 2 * P))


def terms_width(N1, P):
    """Doubles of a site's `out_terms`: [l1 (N1) | l2 (N1) | m (P) | L packed by rows | proposal draws (N1 x P)]."""
    return 2 * N1 + P + P * (P + 1) // 2 + N1 * P


def cut_terms(row, N1, P):
    """A site's `out_terms` as a dict: l1, l2 (N1), m (P), L (P, P) lower, prop (N1, P)."""
    nl = P * (P + 1) // 2
    L = np.zeros((P, P))
    L[np.tril_indices(P)] = row[2 * N1 + P:2 * N1 + P + nl]
    return dict(l1=row[:N1].copy(), l2=row[N1:2 * N1].copy(), m=row[2 * N1:2 * N1 + P].copy(), L=L,
                prop=row[2 * N1 + P + nl:].reshape(N1, P).copy())


# ---- the target

def coefficients(mid, D, gauss, ng, theta):
    """alpha (S, ng) and beta (S, ng or 1, D) from the draws theta (S, P) of a site with ng groups: EPX_NM_ALPHA and
    EPX_NM_BETA (site_params.named_draws), in the dtype of theta."""
    S = theta.shape[0]
    d = site_dims(mid, D, gauss)[0]
    b = theta[:, (1 if gauss else 0):d]
    eta = theta[:, d:d + ng]
    etb = theta[:, d + ng:d + ng + ng * D].reshape(S, ng, D) if mid > 0 else None
    if mid == 0:
        return eta * np.exp(b[:, 0])[:, None], b[:, None, 1:1 + D]
    if mid == 1:
        return eta * np.exp(b[:, 0])[:, None], etb * np.exp(b[:, 1])[:, None, None]
    if mid == 2:
        return eta * np.exp(b[:, 0])[:, None], etb * np.exp(b[:, 1:1 + D])[:, None, :]
    return (b[:, 0][:, None] + eta * np.exp(b[:, 1])[:, None],
            b[:, None, 2:2 + D] + etb * np.exp(b[:, 2 + D:2 + 2 * D])[:, None, :])


def log_target(mid, D, gauss, X, y, groups, mu, Omega, theta):
    """lq (S) of the draws theta (S, P) of ONE site with rows X (n, D), y (n), 0-based group of every row `groups` (n;
    None: one group), cavity (mu, Omega): -1/2 (phi - mu)' Omega (phi - mu) + lprior(lambda) + sum_i ll_i, in the dtype
    of theta."""
    dt = theta.dtype
    X = np.asarray(X, dtype=dt).reshape(-1, D)
    y = np.asarray(y, dtype=dt)
    n = X.shape[0]
    groups = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    ng = int(groups.max()) + 1 if n else 1
    d, P = site_dims(mid, D, gauss, ng)
    if theta.shape[1] != P:
        raise ValueError("theta: (S, {}) for {} groups".format(P, ng))
    alpha, beta = coefficients(mid, D, gauss, ng, theta)
    f = np.empty((theta.shape[0], n), dtype=dt)
    for g in range(ng):
        rows = np.nonzero(groups == g)[0]
        f[:, rows] = alpha[:, g][:, None] + beta[:, g if beta.shape[1] > 1 else 0, :].dot(X[rows].T)
    with np.errstate(all='ignore'):
        if gauss:
            ls = theta[:, :1]
            ll = dt.type(-0.5) * _log_2pi(dt.type) - ls - dt.type(0.5) * np.square((y - f) / np.exp(ls))
        else:
            ll = y * f - (np.maximum(f, 0) + np.log1p(np.exp(-np.abs(f))))
        dphi = theta[:, :d] - np.asarray(mu, dtype=dt)
        quad = np.einsum('si,ij,sj->s', dphi, np.asarray(Omega, dtype=dt), dphi)
        lam = theta[:, d:]
        lprior = -np.abs(lam).sum(axis=1) if mid == 4 else dt.type(-0.5) * np.square(lam).sum(axis=1)
        return dt.type(-0.5) * quad + lprior + ll.sum(axis=1)


# ---- the proposal

def proposal_normals(seed, label, N2, P):
    """z (N2, P), float64: z[r, e] the standard normal of element e at counter (r, K_BRIDGE, e >> 1, 0) under key (seed,
    label): cosine of the Box-Muller pair for even e, sine for odd e."""
    key = _newgroup.make_key(seed, label)
    z = np.empty((N2, P))
    r = np.arange(N2, dtype=np.uint64)
    for p in range((P + 1) // 2):
        u1, u2 = _newgroup.rng_u2(key, r, K_BRIDGE, p, 0)
        rad, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586476925286766559 * u2
        z[:, 2 * p] = rad * np.cos(ang)
        if 2 * p + 1 < P:
            z[:, 2 * p + 1] = rad * np.sin(ang)
    return z


def cholesky_lower(C):
    """The lower Cholesky factor of C in its dtype, or None where a pivot is not finite or numerically <= 0: at most
    P 2^-50 C_jj, what rounding alone leaves of an exact zero."""
    C = np.array(C)
    P = C.shape[0]
    L = np.zeros_like(C)
    tiny = C.dtype.type(P) * C.dtype.type(2.0 ** -50)
    for j in range(P):
        piv = C[j, j] - np.dot(L[j, :j], L[j, :j])
        if not (piv > tiny * C[j, j] and np.isfinite(piv)):
            return None
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = (C[j + 1:, j] - L[j + 1:, :j].dot(L[j, :j])) / L[j, j]
    return L


def solve_lower(L, B):
    """L^-1 B (P, n) by forward substitution, in the dtype of L."""
    V = np.zeros_like(B)
    for i in range(L.shape[0]):
        V[i] = (B[i] - L[i, :i].dot(V[:i])) / L[i, i]
    return V


def fit_proposal(thetaF):
    """(m, L) of the draws thetaF (|F|, P): the mean, and the lower Cholesky factor of the centred scatter / (|F| - 1)
    (None where the factorisation fails)."""
    with np.errstate(all='ignore'):
        m = thetaF.mean(axis=0)
        c = thetaF - m
        return m, cholesky_lower(c.T.dot(c) / thetaF.dtype.type(thetaF.shape[0] - 1))


# ---- the bridge

def _lse(v):
    top = v.max()
    return top + np.log(np.exp(v - top).sum())


def _lse2(a, b):
    top = np.maximum(a, b)
    return top + np.log(np.exp(a - top) + np.exp(b - top))


def bridge(l1, l2):
    """(rho, rho_0, iterations) of Meng & Wong's optimal bridge from the terms l1 (N1) and l2 (N2), in log space."""
    dt = l1.dtype.type
    N1, N2 = l1.shape[0], l2.shape[0]
    ls1, ls2 = np.log(dt(N1) / dt(N1 + N2)), np.log(dt(N2) / dt(N1 + N2))
    rho0 = _lse(l2) - np.log(dt(N2))
    rho = rho0
    for t in range(1, MAX_ITERS + 1):
        b = ls2 + rho
        nxt = (_lse(l2 - _lse2(ls1 + l2, b)) - np.log(dt(N2))) - (_lse(-_lse2(ls1 + l1, b)) - np.log(dt(N1)))
        done = abs(nxt - rho) <= TOL
        rho = nxt
        if done:
            return rho, rho0, t
    return rho, rho0, MAX_ITERS + 1


def relative_mse(l1, l2, rho):
    """EPX_EV_RE2: Var(f2) / (N2 mean(f2)^2) + Var(f1) / (N1 mean(f1)^2) with divisor N - 1, the draws of both sets
    taken as independent (the chains' autocorrelation is not in it)."""
    dt = l1.dtype.type
    N1, N2 = l1.shape[0], l2.shape[0]
    s1, s2 = dt(N1) / dt(N1 + N2), dt(N2) / dt(N1 + N2)
    f1 = dt(1) / (s1 * np.exp(l1 - rho) + s2)
    e2 = np.exp(l2 - rho)
    f2 = e2 / (s1 * e2 + s2)
    return f2.var(ddof=1) / (dt(N2) * f2.mean() ** 2) + f1.var(ddof=1) / (dt(N1) * f1.mean() ** 2)


def site_evidence_host(mid, D, gauss, X, y, groups, mu, Omega, theta, chains, seed, label, proposal=None):
    """(record (EV_COUNT), terms) of ONE site: theta (S, P) its draws in the device's order (its own P coordinates),
    `chains` chains; X (n, D), y (n), groups (n; None: one group) its rows; (mu, Omega) its cavity; label = site0 + k the
    stream's chain.  proposal = (m, L) injects a proposal instead of fitting one to F.  terms: dict of l1, l2 (N1), m
    (P), L (P, P), prop (N2, P), the last three None where the factorisation failed.  Works in the dtype of theta."""
    theta = np.asarray(theta)
    if theta.dtype != np.longdouble:
        theta = theta.astype(np.float64)
    dt = theta.dtype.type
    S, P = theta.shape
    check_sizes(S, chains, P, D)
    F, E = split(S, chains)
    N1 = E.shape[0]
    rec = np.full(EV_COUNT, np.nan, dtype=theta.dtype)
    rec[EV_ITERS], rec[EV_N1] = 0, N1
    m, L = (np.asarray(proposal[0], dtype=theta.dtype), np.asarray(proposal[1], dtype=theta.dtype)) \
        if proposal is not None else fit_proposal(theta[F])
    if L is None:
        return rec, dict(l1=None, l2=None, m=m, L=None, prop=None)
    z = proposal_normals(seed, label, N1, P).astype(theta.dtype)
    prop = m + z.dot(L.T)
    const = np.log(np.diag(L)).sum() + dt(P) / dt(2) * _log_2pi(dt)
    with np.errstate(all='ignore'):
        v = solve_lower(L, (theta[E] - m).T)
        lg1 = dt(-0.5) * np.square(v).sum(axis=0) - const
        lg2 = dt(-0.5) * np.square(z).sum(axis=1) - const
        l1 = log_target(mid, D, gauss, X, y, groups, mu, Omega, theta[E]) - lg1
        l2 = log_target(mid, D, gauss, X, y, groups, mu, Omega, prop) - lg2
    terms = dict(l1=l1, l2=l2, m=m, L=L, prop=prop)
    if not (np.all(np.isfinite(l1)) and np.all(np.isfinite(l2))):
        return rec, terms
    rho, rho0, iters = bridge(l1, l2)
    rec[EV_LOGZ], rec[EV_LOGZ_IS], rec[EV_ITERS] = rho, rho0, iters
    rec[EV_RE2] = relative_mse(l1, l2, rho)
    rec[EV_KHAT] = _loo._psis_row(-l2)[1]
    return rec, terms


# ---- from the sites' values to log Z_EP

def log_partition(Q, r):
    """Phi(Q, r) = 1/2 r' Q^-1 r - 1/2 log det Q + (d / 2) log 2 pi: the log normaliser of exp(-1/2 x' Q x + r' x)."""
    Q = np.asarray(Q, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    L = np.linalg.cholesky(Q)
    v = np.linalg.solve(L, r)
    return 0.5 * v.dot(v) - np.log(np.diag(L)).sum() + 0.5 * Q.shape[0] * _LOG_2PI


def site_log_z(logz, Omega, n_lat, mid):
    """log Z_k = EV_LOGZ + 1/2 log det Omega - (d / 2) log 2 pi - c_lat: the site's normaliser against the NORMALISED
    cavity and the normalised prior of its n_lat latents, c_lat = (n_lat / 2) log 2 pi (m1..m4, standard normal) or n_lat
    log 2 (m5, standard Laplace)."""
    Omega = np.asarray(Omega, dtype=np.float64)
    c_lat = n_lat * math.log(2.0) if mid == 4 else 0.5 * n_lat * _LOG_2PI
    return logz + np.log(np.diag(np.linalg.cholesky(Omega))).sum() - 0.5 * Omega.shape[0] * _LOG_2PI - c_lat


def combine_parts(Q, r, Q0, r0, log_zk, phi_cav):
    """log Z_EP from the sites' log Z_k (K) and the log normalisers of their cavities phi_cav (K) = Phi(Q - Qi_k, r -
    ri_k): what `combine` adds up, for a caller that holds the sites of its own rank only."""
    pq = log_partition(Q, r)
    return float(pq - log_partition(Q0, r0) + np.sum(np.asarray(log_zk) + np.asarray(phi_cav) - pq))


def combine(Q, r, Q0, r0, Qi, ri, log_zk):
    """log Z_EP = Phi(Q, r) - Phi(Q0, r0) + sum_k [log Z_k + Phi(Q - Qi_k, r - ri_k) - Phi(Q, r)] from the global
    approximation (Q, r), the prior (Q0, r0), the sites Qi (d, d, K), ri (d, K) and the sites' log Z_k (K)."""
    Q, r = np.asarray(Q, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return combine_parts(Q, r, Q0, r0, log_zk,
                         [log_partition(Q - Qi[:, :, k], r - ri[:, k]) for k in range(len(log_zk))])
