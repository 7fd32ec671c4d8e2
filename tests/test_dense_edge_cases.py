"""(no device) The case table of the dense-kernel edge tests, dense_edge_cases.py, and its host statement.

 * The edges: every dimension of the table has the tile count, slice count, leading dimension and work-matrix place it
   is in the table for.  The latter two are read from the library's own DensePlan (tests/update_plan_probe.hip, linked with
   libepx.so), so that the LDS / workspace switch cannot move away from the cases unnoticed; the tile and slice counts live
   inside the kernels and are held only against dense_edge_cases.edges(), a restatement of dense.hip's 16 and 256.
 * The reference alone stays inside the bound: with LAPACK (scipy.linalg, oracle.ep_oracle) IN THE DEVICE'S PLACE every
   case passes the very checks test_gpu_dense_edges.py applies to the device -- flags, exact properties and
   |LAPACK - host64| <= max(100 x max|host64 - host_longdouble|, 1e-12 x scale).  A case that did not would leave the
   table here; the bound is never widened on the GPU.
 * The yardstick: longdouble lambda_min against mpmath.eigsy at 40 digits (d <= 17) and against the recorded fixture
   tests/golden/dense_edge_lambda.npz (d >= 255).
 * The flag cases (not positive definite; S = d + 2) give the flags they state in both dtypes (inside the checks).

lapack_ratios() returns the largest LAPACK error / bound per kernel and d; test_gpu_dense_edges.py writes them beside the
device's into the margins file."""

import subprocess

import numpy as np
import pytest
import scipy.linalg as sl

import dense_edge_cases as dc
from oracle import ep_oracle as eo
from test_tree_endings_cases import _build_probe

LAPACK = {}                              # (kernel, d) -> largest error / bound with LAPACK in the device's place


def _keep(kernel, d, r):
    LAPACK[(kernel, d)] = max(LAPACK.get((kernel, d), 0.0), r)


# ------------------------------------------------------------------ the edges
def test_the_table_is_the_one_stated():
    assert dc.DIMS == [2, 3, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 99, 100, 101, 128, 255, 256, 257, 258]
    assert sorted(dc.EDGES) == dc.DIMS and set(dc.COND_DIMS) <= set(dc.DIMS)
    for d, (nt, nsl, where, ld) in dc.EDGES.items():
        assert (nt, nsl, ld) == dc.edges(d), d
    # what the dimensions are in the table for
    assert [dc.EDGES[d][0] for d in (15, 16, 17, 32, 33, 48, 49, 64, 65)] == [1, 1, 2, 2, 3, 3, 4, 4, 5]
    assert [dc.EDGES[d][1] for d in (2, 16, 255, 256, 257)] == [2, 16, 1, 1, 1] and dc.BLOCK // 2 == 128 and dc.BLOCK // 257 == 0
    assert all((dc.EDGES[d][3] == d) == (d % 2 == 1) for d in dc.DIMS)
    for where in ('lds', 'workspace'):                             # both parities on both sides of the switch
        assert {d % 2 for d in dc.DIMS if dc.EDGES[d][2] == where} == {0, 1}
        assert {d % 2 for d in dc.COND_DIMS if dc.EDGES[d][2] == where} == {0, 1}
    for d in dc.DIMS:                                              # S % 4: every residue at every d, with both estimators
        for est in dc.ESTIMATORS:
            assert {S % 4 for S, e, _ in dc.moment_cases(d) if e == est and S <= d + 6} == {0, 1, 2, 3}, (d, est)
            assert [S for S, e, _ in dc.moment_cases(d) if e == est and S != 403][:4] == [d + 3, d + 4, d + 5, d + 6]
        assert all(fams == (['mixed', 'shifted', 'scaled'] if d in dc.COND_DIMS else ['mixed'] * 3)
                   for S, _, fams in dc.moment_cases(d) if S != d + 2)
        assert (d + 2, 'sample', ['mixed'] * 3) in dc.moment_cases(d)
    assert all((403, est, ['mixed', 'shifted', 'scaled']) in dc.moment_cases(d) for d in dc.SLICE_DIMS for est in ('sample', 'olse'))
    assert [dc.slices(K) for K in dc.SUM_K] == [(1, 1, 0), (1, 63, 0), (32, 2, 0), (32, 3, 10), (32, 4, 7)]


def test_the_places_are_the_librarys(tmp_path):
    exe = _build_probe(tmp_path, 'update_plan_probe')
    for d in [1] + dc.DIMS:
        ld, slot, in_lds, lds_bytes, ws = (int(w) for w in subprocess.check_output([exe, 'plan', str(d), '3']).decode().split())
        assert ld == d | 1 and slot == 2 * d * ld + 4 * ld, d
        if d in dc.EDGES:
            assert (ld, 'lds' if in_lds else 'workspace') == (dc.EDGES[d][3], dc.EDGES[d][2]), d
        assert (lds_bytes, ws) == ((slot * 8, 0) if in_lds else (0, 3 * slot)), d
    assert dc.EDGES[99][2] == 'lds' and dc.EDGES[100][2] == 'workspace'


# ------------------------------------------------------------------ the matrices are what they say
@pytest.mark.parametrize('d', dc.COND_DIMS)
def test_the_families_have_their_spectra(d):
    for f in dc.FAMILIES:
        A = dc.matrix(f, d, 0)
        assert np.array_equal(A, A.T) and A.shape == (d, d)
        ev, want = np.linalg.eigvalsh(A), np.sort(dc.spectrum(f, d))
        assert np.abs(ev - want).max() <= 1e-13 * np.abs(want).max() * d, f
        assert (ev[0] < 0) == (f in dc.NOT_PD)
        if f == 'diagonal':
            assert np.array_equal(A, np.diag(np.diag(A))) and dc.gershgorin(A) == (1.0, 10.0)
    S, P = dc.olse_inputs(d, ['linear'] * 3, 'near')
    for i in range(3):                                             # near, not exact, proportionality
        inv = np.linalg.inv(S[i])
        c = np.sum(inv * P[i]) / np.sum(P[i] * P[i])
        assert 1e-5 < np.linalg.norm(inv - c * P[i]) / np.linalg.norm(inv) < 1e-2


def test_the_draw_families():
    for d in dc.DRAW_DIMS:
        x = dict((f, dc.draws(f, d + 5, d, 1)) for f in ('mixed', 'shifted', 'scaled'))
        sd = x['mixed'].std(axis=0)
        assert np.all(np.abs(x['shifted'].mean(axis=0)) > 5e3 * sd) and np.all(np.abs(x['mixed'].mean(axis=0)) < 10 * sd)
        assert x['scaled'][:, -1].std() < 1e-5 * x['scaled'][:, 0].std()


# ------------------------------------------------------------------ LAPACK in the device's place
@pytest.mark.parametrize('d', dc.INVERT_DIMS)
def test_invert_reference_holds_lapack(d):
    for name, fams in dc.invert_batches(d):
        for cho in (False, True):
            A, b, rows = ref = dc.invert_reference(d, name, fams, cho)
            got_A, got_b, info = A.copy(), b.copy(), np.zeros(3, dtype=int)
            for i in range(3):
                try:
                    if cho:
                        if np.any(np.diag(A[i]) == 0.0):
                            raise sl.LinAlgError
                        c = (np.triu(A[i]), False)
                    else:
                        c = sl.cho_factor(A[i], lower=False)
                    inv, potri_info = sl.lapack.dpotri(c[0], lower=0)
                    assert potri_info == 0
                    got_A[i] = np.triu(inv) + np.triu(inv, 1).T
                    got_b[i] = sl.cho_solve(c, b[i])
                except sl.LinAlgError:
                    info[i] = 1
            _keep('k_invert', d, dc.invert_check('d=%d %s cho=%d' % (d, name, cho), ref, got_A, got_b, info))
            assert [r[0][2] for r in rows] == [int(f in dc.NOT_PD) for f in fams]


@pytest.mark.parametrize('with_prior', [False, True])
@pytest.mark.parametrize('d', dc.DIMS)
def test_olse_reference_holds_lapack(d, with_prior):
    for name, fams, prior in dc.olse_batches(d):
        if (prior is not None) != with_prior:
            continue
        S, P, n, rows = ref = dc.olse_reference(d, name, fams, prior)
        got = np.stack([eo.olse(S[i], n, None if P is None else P[i]) for i in range(3)])
        _keep('k_olse', d, dc.olse_check('d=%d %s' % (d, name), ref, got, np.zeros(3, dtype=int)))


@pytest.mark.parametrize('est', dc.ESTIMATORS)
@pytest.mark.parametrize('d', dc.DIMS)
def test_moments_reference_holds_lapack(d, est):
    for S, est, fams in [c for c in dc.moment_cases(d) if c[1] == est]:
        samp, Q, r, rows = ref = dc.moments_reference(d, S, est, fams)
        got = []
        for k in range(3):
            dQi, dri, mt, scatter, ok = eo.tilted_moments(samp[:, :, k], Q, r, est)
            got.append((mt, scatter, dQi, dri, ok))
        worst = dc.moments_check('d=%d S=%d %s' % (d, S, est), ref, got)
        assert all(h[4] and w[4] for h, w in rows)                  # (every draw set of the table gives an estimate)
        _keep('k_moments', d, max(worst.values()))


@pytest.mark.parametrize('d', dc.DIMS)
def test_cavity_reference_holds_lapack(d):
    for name, fams in dc.cavity_batches(d):
        Q, r, Qi, ri, rows = dc.cavity_reference(d, name, fams)
        got = [eo.cavity(Q, r, Qi[k], ri[k]) for k in range(3)]
        _keep('k_cavity', d, dc.cavity_check('d=%d %s' % (d, name), rows, got))
        assert [h[2] for h, w in rows] == [f not in dc.NOT_PD for f in fams]


@pytest.mark.parametrize('d', dc.DIMS)
def test_global_reference_holds_lapack(d):
    for f in dc.global_families(d):
        Q, r, h, w = ref = dc.global_reference(d, f)
        if f in dc.NOT_PD:
            assert not h[2] and not w[2]
            with pytest.raises(eo.NotPosDef):
                eo.invert_normal_params(Q, r)
            continue
        S, m = eo.invert_normal_params(Q, r)
        _keep('k_global', d, dc.global_check('d=%d %s' % (d, f), ref, S, m))


@pytest.mark.parametrize('d', dc.DIMS)
def test_lambda_min_reference_holds_lapack(d):
    for name, thresh, fams, expected in dc.force_calls(d):
        for df in dc.DFS:
            ref = dc.force_reference(d, name, fams, df)
            A = dc.force_matrices(d, fams, df)
            ev = [sl.eigvalsh(A[k], subset_by_index=(0, 0))[0] for k in range(4)]
            _keep('k_force_pd', d, dc.force_check('d=%d %s df=%g' % (d, name, df), ref, thresh, expected, ev,
                                                  [e < thresh for e in ev]))
            Qi, dQi = dc.force_inputs(d, fams, df)
            assert all(np.abs(dQi[k]).max() > 0 for k in range(4))


# ------------------------------------------------------------------ the yardstick
def _as_mp(x):
    import mpmath as mp
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi)))     # (a longdouble is the exact sum of two doubles)


@pytest.mark.parametrize('d', [2, 3, 15, 16, 17])
def test_longdouble_lambda_min_against_mpmath(d):
    import mpmath as mp
    mp.mp.dps = 40
    eps = float(np.finfo(np.longdouble).eps)
    for name, thresh, fams, expected in dc.force_calls(d):
        A = dc.force_matrices(d, fams, 0.37, np.longdouble)
        for k in range(4):
            exact = mp.eigsy(mp.matrix([[_as_mp(v) for v in row] for row in A[k]]), eigvals_only=True)[0]
            norm = float(np.linalg.norm(A[k].astype(np.float64), 2))
            for lam in (dc.lambda_min(A[k]), dc.force_reference(d, name, fams, 0.37)[k][1]):    # plain and bracketed
                assert abs(_as_mp(lam) - exact) <= 4 * eps * norm, (d, name, k, float(abs(_as_mp(lam) - exact)) / (eps * norm))


def test_longdouble_lambda_min_against_the_fixture():
    """The recorded values against a fresh computation.  The matrices come from seeds through np.linalg.qr, and another
    LAPACK build may round them differently by a few float64 eps x norm: the fixture is held to that, 64 eps_float64 x norm
    (Weyl), which is four orders below the 1e-12 x norm floor of the bound it serves; the bracketed bisection itself is held
    to longdouble resolution on the matrix of THIS run."""
    d, (name, thresh, fams, expected) = 257, dc.force_calls(257)[1]
    ref = dc.force_reference(d, name, fams, 0.37)
    eps, eps64 = float(np.finfo(np.longdouble).eps), float(np.finfo(np.float64).eps)
    for k in (1, 3):                                               # lambda_min = 1e-5 and 1e-12 under norms of 1e5 and 1e3
        lam64, wide, norm = ref[k]
        fresh = dc.lambda_min_wide(d, fams, 0.37, k, lam64)
        assert abs(fresh - wide) <= 64 * eps64 * norm, k
        A = dc.force_matrices(d, fams, 0.37, np.longdouble)[k]
        assert dc.lambda_min_within(A, fresh, 8 * eps * norm) and not dc.lambda_min_within(A, fresh + 64 * eps * norm, 8 * eps * norm)


def lapack_ratios():
    """{(kernel, d): largest LAPACK error / bound}: runs what has not run yet in this process."""
    for d in dc.INVERT_DIMS:
        if ('k_invert', d) not in LAPACK:
            test_invert_reference_holds_lapack(d)
    for kernel, fn in (('k_olse', test_olse_reference_holds_lapack), ('k_moments', test_moments_reference_holds_lapack),
                       ('k_cavity', test_cavity_reference_holds_lapack), ('k_global', test_global_reference_holds_lapack),
                       ('k_force_pd', test_lambda_min_reference_holds_lapack)):
        for d in dc.DIMS:
            if (kernel, d) not in LAPACK:
                if kernel == 'k_olse':
                    fn(d, False), fn(d, True)
                elif kernel == 'k_moments':
                    fn(d, 'sample'), fn(d, 'olse')
                else:
                    fn(d)
    return dict(LAPACK)
