"""The case table and the host statement of the dense-kernel edge tests (plain helper, NumPy only, no device, no torch, no
tests): test_dense_edge_cases.py (no device) and test_gpu_dense_edges.py (device) share it.

csrc/dense.hip runs one d x d problem per workgroup of 256 threads.  What its kernels decide from d, written ONCE, here
(EDGES holds the values the cases claim; the CPU test reads ld and the place of the work matrices from the library's own
DensePlan; nt and nsl live inside the kernels and are NOT held against the library: edges() below restates dense.hip's 16 and
256, and whoever changes them there changes them here):

    ld     = d | 1                       leading dimension of the work matrices: odd d has no padding row, even d one
    slot   = 2 d ld + 4 ld doubles       per workgroup: dynamic LDS while it fits (d <= 99), else slot blockIdx.x of a workspace
    nt     = ceil(d / 16)                16 x 16 MFMA tiles a side of the scatter matrix, nt (nt + 1) / 2 tiles in all
    nsl    = min(max(256 // d, 1), d)    slices of the draw index in draw_mean
    S % 4                                the scatter consumes four draws per MFMA: a partial last group is masked

The host statements below work IN THE DTYPE OF THEIR INPUT (float64 or np.longdouble) with vectorised column loops: the
float64 run is the reference a device result is compared with, |float64 - longdouble| measures that reference's own error,
and the bound of every comparison is (bound())

    |device - host64| <= max(100 x max|host64 - host_longdouble|, 1e-12 x scale)

both maxima over the output array of the case, scale = max|host64| (the matrix 2-norm for an eigenvalue).  It is the rule of
test_gpu_reweight.derived_check and test_gpu_loo._psis_check.

Matrices are Q diag(ev) Q' of a seeded orthogonal Q, symmetrised; FAMILIES names the spectra.  `python
tests/golden/make_dense_golden.py` records the longdouble lambda_min of the large force-pd cases (tests/golden/dense_edge_lambda.npz)."""

import os

import numpy as np

BLOCK = 256                              # threads of a workgroup of every kernel in csrc/dense.hip
DIMS = [2, 3, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 99, 100, 101, 128, 255, 256, 257, 258]
COND_DIMS = [2, 17, 32, 99, 100, 257]    # dimensions that get the conditioning families
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dense_edge_lambda.npz')
GOLDEN_FROM = 255                        # longdouble lambda_min is read from GOLDEN from this d on (about 1 s each and more)

# d: (nt, nsl, where the work matrices are, ld) -- what each dimension is in the table for
EDGES = {
    2: (1, 2, 'lds', 3),        # 256 // 2 = 128 slices clamped to d
    3: (1, 3, 'lds', 3),        # odd: ld == d
    15: (1, 15, 'lds', 15),     # one tile, one column short
    16: (1, 16, 'lds', 17),     # one exact tile; nsl == d == 256 // d
    17: (2, 15, 'lds', 17),     # a second tile with one row
    31: (2, 8, 'lds', 31),
    32: (2, 8, 'lds', 33),      # two exact tiles
    33: (3, 7, 'lds', 33),      # a nearly empty last tile
    48: (3, 5, 'lds', 49),      # three exact tiles
    49: (4, 5, 'lds', 49),
    64: (4, 4, 'lds', 65),
    65: (5, 3, 'lds', 65),
    99: (7, 2, 'lds', 99),      # the last dimension in LDS
    100: (7, 2, 'workspace', 101),   # the first in the workspace, padded
    101: (7, 2, 'workspace', 101),   # the workspace without padding
    128: (8, 2, 'workspace', 129),
    255: (16, 1, 'workspace', 255),  # one thread short of a column each
    256: (16, 1, 'workspace', 257),  # one column per thread, nsl = 1
    257: (17, 1, 'workspace', 257),  # 256 // d = 0 clamped to 1; potri's columns wrap
    258: (17, 1, 'workspace', 259),
}


def edges(d):
    """(nt, nsl, ld) by the rules of csrc/dense.hip."""
    return (d + 15) // 16, min(max(BLOCK // d, 1), d), d | 1


# ---------------------------------------------------------------- the host statement
def cholesky(A):
    """(L, ok): the lower Cholesky factor of A from its lower triangle, column by column; ok is False at the first pivot that
    is <= 0, NaN or inf (block_potrf's rule) and L is then unfinished."""
    A = np.asarray(A)
    d = A.shape[0]
    L = np.zeros_like(A)
    for j in range(d):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not (c[0] > 0) or not np.isfinite(c[0]):
            return L, False
        L[j, j] = np.sqrt(c[0])
        L[j + 1:, j] = c[1:] / L[j, j]
    return L, True


def solve(L, b):
    """(L L')^-1 b."""
    x = np.array(b, dtype=L.dtype)
    d = L.shape[0]
    for j in range(d):
        x[j] /= L[j, j]
        x[j + 1:] -= L[j + 1:, j] * x[j]
    for j in range(d - 1, -1, -1):
        x[j] /= L[j, j]
        x[:j] -= L[j, :j] * x[j]
    return x


def inverse(L):
    """(L L')^-1 = L^-T L^-1, the upper triangle a copy of the lower."""
    d = L.shape[0]
    Z = np.eye(d, dtype=L.dtype)                         # L^-1 by forward substitution on all columns
    for j in range(d):
        Z[j, :j + 1] /= L[j, j]
        Z[j + 1:, :j + 1] -= np.outer(L[j + 1:, j], Z[j, :j + 1])
    M = np.tril(Z.T @ Z)
    return M + np.tril(M, -1).T


def invert(A, b=None, cho_form=False):
    """util.invert_normal_params: (A^-1, A^-1 b, info).  cho_form: A holds the UPPER factor U, A = U'U; info = 1 for a matrix
    that is not positive definite (cho_form: a diagonal entry of the factor that is 0 or not finite), and A, b come back as
    they were."""
    A = np.asarray(A)
    if cho_form:
        L, ok = np.triu(A).T.copy(), bool(np.all(np.diag(A) != 0) and np.all(np.isfinite(np.diag(A))))
    else:
        L, ok = cholesky(A)
    if not ok:
        return A.copy(), None if b is None else np.array(b, dtype=A.dtype), 1
    return inverse(L), None if b is None else solve(L, b), 0


def olse(S, n, P=None):
    """util.olse (util.py:128-194 of the reference): (estimate, info)."""
    S = np.asarray(S)
    d = S.shape[0]
    out, _, info = invert(S)
    if info:
        return out, 1
    tr = np.trace(out)
    tr2, f2 = tr * tr, np.sum(out * out)
    if P is None:
        alpha = 1 - (d + tr2 / (f2 - tr2 / d)) / n
        beta = tr * (1 - S.dtype.type(d) / n - alpha)
        out = alpha * out
        out[np.diag_indices(d)] += beta / d
    else:
        P = np.asarray(P, dtype=S.dtype)
        f2p, tsp = np.sum(P * P), np.sum(out * P)
        alpha = 1 - (d + tr2 * f2p / (f2 * f2p - tsp * tsp)) / n
        beta = (tsp / f2p) * (1 - S.dtype.type(d) / n - alpha)
        out = alpha * out + beta * P
    return out, 0


def cavity(Q, r, Qi, ri, dQi=None, dri=None, df=0.0):
    """Worker.cavity on the site Qi (+ df dQi), ri (+ df dri): (Om, mu, ok); mu is r - ri unsolved where Om is not positive
    definite."""
    Q = np.asarray(Q)
    t = Q.dtype.type
    q = np.asarray(Qi, dtype=t) if dQi is None else np.asarray(Qi, dtype=t) + t(df) * np.asarray(dQi, dtype=t)
    v = np.asarray(ri, dtype=t) if dri is None else np.asarray(ri, dtype=t) + t(df) * np.asarray(dri, dtype=t)
    Om, vec = Q - q, np.asarray(r, dtype=t) - v
    L, ok = cholesky(Om)
    return Om, solve(L, vec) if ok else vec, ok


def precision_tail(mean, scatter, n, Q, r, est):
    """The precision estimate of n draws' worth from their scatter matrix and mean, and the site update: (dQi, dri, ok)."""
    t = scatter.dtype.type
    d = scatter.shape[0]
    Q, r = np.asarray(Q, dtype=t), np.asarray(r, dtype=t)
    if est == 'sample':
        prec, _, info = invert(scatter)
        if not info:
            ub = t(n) - t(d + 2)
            return prec * ub - Q, (prec @ mean) * ub - r, True
    else:
        prec, info = olse(scatter / t(n), t(n), P=Q)
        if not info:
            return prec - Q, prec @ mean - r, True
    return np.zeros_like(Q), np.zeros_like(r), False


def moments(samp, Q, r, est):
    """The tilted moment stage on the draws samp (S, d): (mean, scatter, dQi, dri, ok); two passes -- the mean, then the
    scatter matrix of the centred draws."""
    samp = np.asarray(samp)
    S = samp.shape[0]
    mean = samp.sum(axis=0) / samp.dtype.type(S)
    C = samp - mean
    scatter = C.T @ C
    return (mean, scatter) + precision_tail(mean, scatter, S, Q, r, est)


def global_moments(Q, r):
    """(S, m, ok) = (Q^-1, Q^-1 r)."""
    S, m, info = invert(Q, r)
    return S, m, not info


def _below(A, s):
    """Whether A - s I has no negative or zero pivot in its LDL' (without pivoting), i. e. s < lambda_min(A): the inertia of
    A - s I counted only as far as lambda_min needs it -- the elimination stops at the first pivot that is not positive,
    until where it is the elimination of a positive definite matrix and stable."""
    d = A.shape[0]
    W = np.tril(A)
    W[np.diag_indices(d)] -= s
    L = np.zeros_like(W)                                 # columns l_j d_j
    D = np.zeros(d, dtype=A.dtype)
    for j in range(d):
        c = W[j:, j] - L[j:, :j] @ (L[j, :j] / D[:j])
        if not c[0] > 0:
            return False
        D[j] = c[0]
        L[j:, j] = c
    return True


def gershgorin(A):
    rad = np.abs(A).sum(axis=1) - np.abs(np.diag(A))
    return (np.diag(A) - rad).min(), (np.diag(A) + rad).max()


def lambda_min(A, start=None):
    """The smallest eigenvalue of the symmetric A by bisection on the inertia of A - s I, from Gershgorin's bounds to the
    resolution of A's dtype.  start = (lo, hi): a bracket to begin with instead (it is verified and widened if wrong)."""
    A = np.asarray(A)
    t = A.dtype.type
    glo, ghi = gershgorin(A)
    span = max(ghi - glo, t(1e-300))
    glo, ghi = glo - t(1e-12) * span - t(1e-300), ghi + t(1e-12) * span + t(1e-300)
    lo, hi = glo, ghi
    if start is not None:
        w = t(start[1]) - t(start[0])
        lo, hi = t(start[0]), t(start[1])
        while lo > glo and not _below(A, lo):
            lo, w = max(lo - w, glo), 2 * w
        while hi < ghi and _below(A, hi):
            hi, w = min(hi + w, ghi), 2 * w
    eps = np.finfo(A.dtype).eps
    norm = max(abs(glo), abs(ghi))
    for _ in range(200):
        mid = (lo + hi) / 2
        if not (lo < mid < hi) or hi - lo <= eps * norm / 8:
            break
        if _below(A, mid):
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def lambda_min_within(A, value, tol):
    """Whether |lambda_min(A) - value| <= tol, by two inertia counts in A's dtype."""
    t = np.asarray(A).dtype.type
    return _below(A, t(value) - t(tol)) and not _below(A, t(value) + t(tol))


def bound(host, wide, scale=None):
    """The bound of a comparison with `host` (float64), whose own error `wide` (longdouble) measures."""
    host = np.asarray(host, dtype=np.float64)
    ref = float(np.max(np.abs(host - np.asarray(wide)))) if host.size else 0.0
    if scale is None:
        scale = float(np.max(np.abs(host))) if host.size else 0.0
    return max(100.0 * ref, 1e-12 * scale)


def ratio(got, host, wide, scale=None):
    """largest |got - host| / bound(host, wide)."""
    b = bound(host, wide, scale)
    err = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(host, dtype=np.float64))))
    return err / b if b > 0.0 else (0.0 if err == 0.0 else np.inf)


# ---------------------------------------------------------------- matrices
FAMILIES = ('linear', 'log1e6', 'log1e10', 'diagonal', 'cluster', 'negative', 'tiny')
NOT_PD = ('negative',)
INVERTIBLE = ('linear', 'log1e6', 'log1e10', 'diagonal', 'cluster')     # (tiny: kappa = 1e15, no bound to hold an inverse to)


def spectrum(family, d):
    if family in ('linear', 'diagonal'):
        return np.linspace(1.0, 10.0, d) if d > 1 else np.array([2.5])
    if family.startswith('log'):
        k = float(family[3:])
        return np.logspace(-0.5 * np.log10(k), 0.5 * np.log10(k), d) if d > 1 else np.array([3.0])
    ev = np.linspace(1.0, 2.0, d)
    if family == 'cluster':                  # three (d < 4: d - 1) eigenvalues 1e-6 (1 + 1e-9 j) under a bulk in [1, 2]
        n = min(3, d - 1)
        ev[:n] = 1e-6 * (1.0 + 1e-9 * np.arange(n))
    elif family == 'negative':               # one eigenvalue -0.3: not positive definite
        ev[0] = -0.3
    elif family == 'tiny':                   # lambda_min = 1e-12 under a bulk in [1e-3, 1e3]
        ev = np.logspace(-3.0, 3.0, d)
        ev[0] = 1e-12
    else:
        raise ValueError(family)
    return ev


def _seed(*parts):
    h = 2166136261
    for p in parts:
        for ch in str(p) + '|':
            h = ((h ^ ord(ch)) * 16777619) & 0xffffffff
    return h


def orthogonal(d, seed):
    q, r = np.linalg.qr(np.random.RandomState(seed).randn(d, d))
    return q * np.sign(np.diag(r))


def matrix(family, d, seed):
    """(d, d) float64, exactly symmetric, with (up to rounding) the spectrum of the family."""
    ev = spectrum(family, d)
    if d == 1:
        ev = ev + seed                           # (one entry: the seed has to tell the matrices of a batch apart)
    if family == 'diagonal':
        return np.diag(np.random.RandomState(_seed('diag', d, seed)).permutation(ev))
    q = orthogonal(d, _seed(family, d, seed))
    A = (q * ev).dot(q.T)
    return 0.5 * (A + A.T)


def symmetric_noise(d, seed, size=1.0):
    n = np.random.RandomState(_seed('noise', d, seed)).randn(d, d)
    return size * 0.5 * (n + n.T) / np.sqrt(max(d, 1))


def vector(d, seed):
    return np.random.RandomState(_seed('vec', d, seed)).randn(d)


def families_of(d):
    return INVERTIBLE if d in COND_DIMS else ('linear',)


# ---------------------------------------------------------------- A. invert: batches of three different matrices
def invert_batches(d):
    """[(name, [three families])]: every batch has three DIFFERENT matrices (seeds 0, 1, 2); the not-PD batch has its
    negative member in the middle."""
    out = [(f, [f, f, f]) for f in families_of(d)]
    if d in COND_DIMS:
        out.append(('negative', ['linear', 'negative', 'log1e6']))
    return out


def invert_inputs(d, fams):
    A = np.stack([matrix(f, d, i) for i, f in enumerate(fams)])
    b = np.stack([vector(d, 10 + i) for i in range(len(fams))])
    return A, b


INVERT_DIMS = [1] + DIMS                 # (d = 1: the stand-alone entries only)


# ---------------------------------------------------------------- B. olse
def olse_n(d):
    return 4 * d + 10


def olse_batches(d):
    """[(name, [three families of S], prior)]: prior None, 'generic' (P at a generic angle to S^-1) or 'near' (S^-1 = c P +
    1e-3 noise: the denominator f2 f2p - tsp^2 loses digits).  Exact proportionality is 0 / 0 in the reference too and is no case."""
    out = []
    for f in families_of(d):
        out.append((f, [f, f, f], None))
        out.append((f + '+P', [f, f, f], 'generic'))
    if d in COND_DIMS:
        out.append(('linear+nearP', ['linear'] * 3, 'near'))
    return out


def olse_inputs(d, fams, prior):
    S = np.stack([matrix(f, d, 20 + i) for i, f in enumerate(fams)])
    if prior is None:
        return S, None
    if prior == 'generic':
        return S, np.stack([matrix('linear', d, 30 + i) for i in range(len(fams))])
    P = []
    for i in range(len(fams)):
        inv = np.linalg.inv(S[i])
        P.append((inv + 1e-3 * np.abs(inv).max() * symmetric_noise(d, 40 + i)) / 1.7)
    return S, np.stack(P)


# ---------------------------------------------------------------- C. moments: draws
DRAW_DIMS = COND_DIMS                    # dimensions that get the draw families besides 'mixed'
ESTIMATORS = ('sample', 'olse')
SLICE_DIMS = [2, 17, 32]                 # ... and S = 403 (the slice loop of draw_mean, many MFMA groups)


def draws(family, S, d, seed):
    """(S, d) float64 draws: 'mixed' as test_gpu_parity.g4_samples mixes them; 'shifted' the same with the shift at 1e4
    standard deviations (cancellation in the centring); 'scaled' with the last coordinate scaled by 1e-6."""
    rng = np.random.RandomState(_seed('draws', d, seed))
    mix = np.eye(d) + 0.3 * rng.randn(d, d) / np.sqrt(d)
    shift = rng.randn(d)
    x = rng.randn(S, d).dot(mix)
    if family == 'shifted':
        shift = 1e4 * np.sign(shift) * (1.0 + np.abs(shift))
    x = x + shift
    if family == 'scaled':
        x[:, -1] *= 1e-6
    elif family not in ('mixed', 'shifted'):
        raise ValueError(family)
    return x


def moment_cases(d):
    """[(S, est, [three draw families])]: S = d + 3 .. d + 6 covers S % 4 at every d, with both estimators; S = d + 2 makes the
    'sample' update exactly -Q, -r; S = 403 at the small dimensions runs the slice loop and many MFMA groups."""
    fams = ['mixed', 'shifted', 'scaled'] if d in DRAW_DIMS else ['mixed'] * 3
    out = [(d + a, est, fams) for a in (3, 4, 5, 6) for est in ESTIMATORS]
    out.append((d + 2, 'sample', ['mixed'] * 3))
    if d in SLICE_DIMS:
        out += [(403, est, fams) for est in ESTIMATORS]
    return out


def moment_inputs(d, S, fams):
    """(samples (S, d, 3) F-ordered, Q, r)."""
    samp = np.asfortranarray(np.stack([draws(f, S, d, 50 + i) for i, f in enumerate(fams)], axis=2))
    return samp, matrix('linear', d, 60), vector(d, 61)


# ---------------------------------------------------------------- D. cavity / E. global
def cavity_batches(d):
    out = [('linear', ['linear'] * 3)]
    if d in COND_DIMS:
        out += [('conditioned', ['log1e6', 'cluster', 'diagonal']), ('negative', ['log1e10', 'negative', 'linear'])]
    return out


def cavity_inputs(d, fams):
    """(Q, r, Qi (3, d, d), ri (3, d)) with Q - Qi[k] of the family fams[k] up to the rounding of one subtraction."""
    Om = [matrix(f, d, 70 + i) for i, f in enumerate(fams)]
    big = max(np.abs(o).max() for o in Om)
    Q = big * matrix('linear', d, 80)
    Qi = np.stack([Q - o for o in Om])
    return Q, vector(d, 81), Qi, np.stack([vector(d, 82 + i) for i in range(len(fams))])


def proposal_inputs(d, K=3):
    """(Q0, r0, Qi, ri, dQi, dri) of a trial whose global Q = Q0 + sum Qi + df sum dQi and cavities are positive definite."""
    Qi = np.stack([0.3 * matrix('linear', d, 90 + k) for k in range(K)])
    dQi = np.stack([symmetric_noise(d, 95 + k, 0.2) for k in range(K)])
    ri = np.stack([vector(d, 100 + k) for k in range(K)])
    dri = np.stack([vector(d, 105 + k) for k in range(K)])
    return matrix('linear', d, 110), vector(d, 111), Qi, ri, dQi, dri


def global_families(d):
    return families_of(d) + (('negative',) if d in COND_DIMS else ())


# ---------------------------------------------------------------- F. force pd
DFS = (1.0, 0.37)
TARGET = 0.5


def force_calls(d):
    """[(name, thresh, [four families], [forced])]: two sites below the threshold and two above it in every call."""
    out = [('plain', 1e-5, ['linear', 'negative', 'diagonal', 'cluster'], [False, True, False, True])]
    if d in COND_DIMS:
        out.append(('conditioned', 1e-4, ['log1e6', 'log1e10', 'linear', 'tiny'], [False, True, False, True]))
    return out


def force_inputs(d, fams, df):
    """(Qi, dQi), each (4, d, d), with Qi + df dQi of the family up to rounding and dQi not zero."""
    A = [matrix(f, d, 120 + k) for k, f in enumerate(fams)]
    dQi = np.stack([symmetric_noise(d, 130 + k, 0.1 * np.abs(a).max()) for k, a in enumerate(A)])
    if 'diagonal' in fams:                       # (keeps the Gershgorin radius of that site zero)
        k = fams.index('diagonal')
        dQi[k] = np.diag(np.diag(dQi[k]))
    return np.stack([a - df * dq for a, dq in zip(A, dQi)]), dQi


def force_matrices(d, fams, df, dtype=np.float64):
    """Qi + df dQi as the statement forms it in `dtype` from the float64 inputs."""
    Qi, dQi = force_inputs(d, fams, df)
    return Qi.astype(dtype) + dtype(df) * dQi.astype(dtype)


def golden_key(d, name, df, k):
    return 'd%d_%s_df%s_k%d' % (d, name, ('%g' % df).replace('.', 'p'), k)


_golden = {}


def force_reference(d, name, fams, df):
    """[(host64 lambda_min, longdouble lambda_min, ||A||_2 bound)] of the four sites; the longdouble value comes from GOLDEN
    from d = GOLDEN_FROM on."""
    A64 = force_matrices(d, fams, df)
    out = []
    for k in range(len(fams)):
        lam = lambda_min(A64[k])
        if d >= GOLDEN_FROM:
            if not _golden:
                with np.load(GOLDEN) as z:
                    _golden.update((key, z[key]) for key in z.files)
            hi, lo = _golden[golden_key(d, name, df, k)]            # a longdouble as the sum of two doubles
            wide = np.longdouble(hi) + np.longdouble(lo)
        else:
            wide = lambda_min_wide(d, fams, df, k, lam)
        out.append((lam, wide, float(np.linalg.norm(A64[k], 2))))
    return out


def lambda_min_wide(d, fams, df, k, near):
    """longdouble lambda_min of site k's matrix, bracketed about the float64 result to save bisections."""
    A = force_matrices(d, fams, df, np.longdouble)[k]
    w = 1e-9 * max(float(np.abs(A).max()), 1e-300)
    return lambda_min(A, start=(near - w, near + w))


# ---------------------------------------------------------------- G. sums
SUM_K = [1, 63, 64, 65, 97]              # nslice is 1 below K = 64 and 32 from there on; K = 65 leaves empty trailing slices
SUM_MODELS = [('m2b_sg', 2), ('m1b_sg', 17)]


def slices(K):
    """(nslice, sites per slice, slices that are empty) as epx_api.hip and k_site_sums_partial cut K sites."""
    nslice = 32 if K >= 64 else 1
    per = -(-K // nslice)
    return nslice, per, sum(1 for b in range(nslice) if b * per >= K)


def mixed_values(shape, seed):
    """Values of mixed sign and magnitude (1e-8 .. 1e8)."""
    rng = np.random.RandomState(_seed('sums', seed))
    return rng.randn(*shape) * 10.0 ** rng.randint(-8, 9, size=shape)


# ---------------------------------------------------------------- references (computed once per process) and checks
# A check takes what the device -- or, in test_dense_edge_cases.py, LAPACK in the device's place -- returned for a case,
# asserts flags, exact properties and the bound, and returns the largest error / bound of the case.
LD = np.longdouble
_memo = {}


def memo(key, make):
    if key not in _memo:
        with np.errstate(all='ignore'):
            _memo[key] = make()
    return _memo[key]


def held(what, got, host, wide, scale=None):
    r = ratio(got, host, wide, scale)
    assert r <= 1.0, '%s: error / bound %.3e (bound %.3e)' % (what, r, bound(host, wide, scale))
    return r


def invert_reference(d, name, fams, cho):
    """(A (3, d, d), b (3, d), [(host64, longdouble)]) of a batch; cho: A holds upper factors, junk below their diagonals,
    and the not-PD member is a factor with a zero on its diagonal."""
    def make():
        A, b = invert_inputs(d, fams)
        if cho:
            U = []
            for i, f in enumerate(fams):
                u = cholesky(A[i] if f not in NOT_PD else matrix('linear', d, 3))[0].T.copy()
                if f in NOT_PD:
                    u[d // 2, d // 2] = 0.0
                U.append(u + np.tril(np.full((d, d), 7.0), -1))
            A = np.stack(U)
        return A, b, [(invert(A[i], b[i], cho), invert(A[i].astype(LD), b[i].astype(LD), cho)) for i in range(len(fams))]
    return memo(('invert', d, name, cho), make)


def invert_check(what, ref, got_A, got_b, got_info):
    A, b, rows = ref
    worst = 0.0
    for i, (h, w) in enumerate(rows):
        assert int(got_info[i]) == h[2] == w[2], (what, i, got_info[i], h[2], w[2])
        if h[2]:
            assert np.array_equal(got_A[i], A[i]) and (got_b is None or np.array_equal(got_b[i], b[i])), (what, i)
            continue
        assert np.array_equal(got_A[i], got_A[i].T), (what, i, 'not symmetric')
        worst = max(worst, held('%s member %d inverse' % (what, i), got_A[i], h[0], w[0]))
        if got_b is not None:
            worst = max(worst, held('%s member %d solve' % (what, i), got_b[i], h[1], w[1]))
    return worst


def olse_reference(d, name, fams, prior):
    def make():
        S, P = olse_inputs(d, fams, prior)
        n = olse_n(d)
        rows = [(olse(S[i], n, None if P is None else P[i]),
                 olse(S[i].astype(LD), n, None if P is None else P[i].astype(LD))) for i in range(len(fams))]
        return S, P, n, rows
    return memo(('olse', d, name), make)


def olse_check(what, ref, got, got_info):
    worst = 0.0
    for i, (h, w) in enumerate(ref[3]):
        assert int(got_info[i]) == h[1] == w[1] == 0, (what, i)
        worst = max(worst, held('%s member %d' % (what, i), got[i], h[0], w[0]))
    return worst


MOMENT_NAMES = ('mean', 'scatter', 'dQi', 'dri')


def moments_reference(d, S, est, fams):
    """(samples, Q, r, [(host64, longdouble)]): each a (mean, scatter, dQi, dri, ok)."""
    def make():
        samp, Q, r = moment_inputs(d, S, fams)
        rows = [(moments(samp[:, :, k], Q, r, est), moments(samp[:, :, k].astype(LD), Q.astype(LD), r.astype(LD), est))
                for k in range(samp.shape[2])]
        return samp, Q, r, rows
    return memo(('moments', d, S, est, tuple(fams)), make)


def moments_check(what, ref, got, sites=None):
    """got: [(mean, scatter, dQi, dri, flag)] per site -> {output: largest error / bound}."""
    samp, Q, r, rows = ref
    S, d = samp.shape[:2]
    worst = dict.fromkeys(MOMENT_NAMES, 0.0)
    for k in (range(len(rows)) if sites is None else sites):
        h, w = rows[k]
        g = got[k]
        assert bool(g[4]) == h[4] == w[4], (what, k, g[4], h[4], w[4])
        if S == d + 2 and h[4]:
            assert np.array_equal(g[2], -Q) and np.array_equal(g[3], -r), (what, k, 'n - d - 2 = 0: the update is -Q, -r')
        for i, name in enumerate(MOMENT_NAMES):
            worst[name] = max(worst[name], held('%s site %d %s' % (what, k, name), g[i], h[i], w[i]))
    return worst


def cavity_reference(d, name, fams):
    def make():
        Q, r, Qi, ri = cavity_inputs(d, fams)
        rows = [(cavity(Q, r, Qi[k], ri[k]), cavity(Q.astype(LD), r.astype(LD), Qi[k].astype(LD), ri[k].astype(LD)))
                for k in range(len(fams))]
        return Q, r, Qi, ri, rows
    return memo(('cavity', d, name), make)


def cavity_check(what, rows, got, exact_Om=True, sites=None):
    """got: [(Om, mu, flag)] per site."""
    worst = 0.0
    for k in (range(len(rows)) if sites is None else sites):
        h, w = rows[k]
        Om, mu, flag = got[k]
        assert bool(flag) == h[2] == w[2], (what, k, flag, h[2], w[2])
        if exact_Om:
            assert np.array_equal(Om, h[0]), (what, k, 'Om is one subtraction')
        else:
            worst = max(worst, held('%s site %d Om' % (what, k), Om, h[0], w[0]))
        if h[2]:
            worst = max(worst, held('%s site %d mu' % (what, k), mu, h[1], w[1]))
        elif exact_Om:
            assert np.array_equal(mu, h[1]), (what, k, 'r - ri is left unsolved')
    return worst


def global_reference(d, family):
    def make():
        Q, r = matrix(family, d, 140), vector(d, 141)
        return Q, r, global_moments(Q, r), global_moments(Q.astype(LD), r.astype(LD))
    return memo(('global', d, family), make)


def global_check(what, ref, S, m):
    Q, r, h, w = ref
    assert h[2] and w[2], what
    assert np.array_equal(S, S.T), (what, 'not symmetric')
    return max(held(what + ' S', S, h[0], w[0]), held(what + ' m', m, h[1], w[1]))


def force_check(what, ref, thresh, expected, got_lambda, got_forced):
    """ref: force_reference(); got_lambda: the smallest eigenvalue the device (or LAPACK) found per site (None: not known,
    an unforced site of the device) -> largest error / bound."""
    worst = 0.0
    for k, (lam, wide, norm) in enumerate(ref):
        b = bound(lam, wide, norm)
        assert abs(lam - thresh) > b and abs(float(wide) - thresh) > b, (what, k, 'the case sits on the threshold')
        assert (lam < thresh) == (float(wide) < thresh) == expected[k] == bool(got_forced[k]), (what, k, lam, got_forced[k])
        if got_lambda[k] is not None:
            worst = max(worst, held('%s site %d lambda_min' % (what, k), got_lambda[k], lam, wide, norm))
    return worst
