"""csrc/dense.hip on the device at the edges the case table tests/dense_edge_cases.py names: exact, nearly empty and
partial MFMA tiles, the last partial group of four draws, the block size 256 (d = 255 .. 258), the LDS / workspace switch at
d = 99 / 100 in both parities of d (ld == d, ld == d + 1), more than one workspace slot, sub-batches with k0 > 0, the slicing
of the site sums about K = 64 -- on well and badly conditioned inputs.  Need a real MI355X.

The device runs through the Python entries only (HipEngine, the _lib entries of util.invert_normal_params / util.olse for
batches) and is held against the float64 host statement of dense_edge_cases.py by the project's rule

    |device - host64| <= max(100 x max|host64 - host_longdouble|, 1e-12 x scale)

per output array of a case (dense_edge_cases.bound), with the flags and the exact properties (symmetry, one subtraction,
untouched bytes) asserted beside it.  test_dense_edge_cases.py (no device) applies the same checks to LAPACK in the device's
place: the reference alone stays inside the bound on every case.

No sampler runs: every test builds contexts of two rows per site.

The largest error / bound per kernel and d measured on an MI355X, and the file's wall time, are in
profiles/dense_edges_margins.txt.

EPX_DENSE_MARGINS=<file>: the figures of the run are written there (profiles/dense_edges_margins.txt is such a file)."""

import math
import os
import time
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dense_edge_cases as dc                                    # noqa: E402
from epstan_amd import _lib, util                                # noqa: E402
from epstan_amd.engine import HipEngine, QI, QI2, DQI            # noqa: E402
from test_gpu_parity import _site_problem                        # noqa: E402

LD = np.longdouble
RECORD = {'worst': {}, 'cases': 0, 't0': time.perf_counter()}
_engines = {}


def _keep(kernel, d, r, cases=1):
    RECORD['worst'][(kernel, d)] = max(RECORD['worst'].get((kernel, d), 0.0), r)
    RECORD['cases'] += cases


def _new_engine(d, K, model='m1b_sg'):
    X, y, k_lim = _site_problem(model, d - 1 if model == 'm1b_sg' else 1, 2, 5, K=K)[:3]
    e = HipEngine(model, X, y, k_lim)
    assert (e.d, e.K) == (d, K)
    return e


def engine(d, K, model='m1b_sg'):
    """The module's context of K sites at dimension d (two rows per site)."""
    if (model, d, K) not in _engines:
        _engines[(model, d, K)] = _new_engine(d, K, model)
    return _engines[(model, d, K)]


@pytest.fixture(scope='module', autouse=True)
def _engines_and_margins():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()
    path = os.environ.get('EPX_DENSE_MARGINS')
    if not path or not RECORD['worst']:
        return
    wall = time.perf_counter() - RECORD['t0']
    from test_dense_edge_cases import lapack_ratios
    lapack = lapack_ratios()
    kernels = ['k_invert', 'k_olse', 'k_moments', 'k_cavity', 'k_cavity(proposal)', 'k_global', 'k_force_pd', 'k_site_sums',
               'k_mix']
    with open(path, 'w') as f:
        f.write('# tests/test_gpu_dense_edges.py: largest error / bound per kernel and d; the bound is max(100 x max|host64 -\n'
                '# host_longdouble|, 1e-12 x scale) over the output array of a case (tests/dense_edge_cases.py: bound), for the sums\n'
                '# (K - 1) 2^-53 sum|x_k| per element (one more rounding per product in k_mix).  "lapack": LAPACK in the\n'
                '# device\'s place (tests/test_dense_edge_cases.py), the same checks.\n')
        f.write('# no case has a widened bound\n')
        f.write('# checked device calls: %d; wall time of the file: %.1f s\n' % (RECORD['cases'], wall))
        slots = sorted(d for (k, d) in RECORD['worst'] if k == 'workspace slots')
        if slots:
            f.write('# 17 blocks on the workspace path keep to their slots (the bytes of every member alone): d = %s\n'
                    % ', '.join(str(d) for d in slots))
        for kern in kernels:
            rows = sorted((d, r) for (k, d), r in RECORD['worst'].items() if k == kern)
            if rows:
                f.write('%s: largest over all d %.2e\n' % (kern, max(r for _, r in rows)))
                for d, r in rows:
                    f.write('  d=%-4d device %.2e%s\n' % (d, r, ' lapack %.2e' % lapack[(kern, d)] if (kern, d) in lapack else ''))


def _sites(stack):
    """(K, d, d) or (K, d) -> (d, d, K) or (d, K) in F order, as set_sites takes them."""
    return np.asfortranarray(np.moveaxis(stack, 0, -1))


def _colmajor(stack):
    """(nb, d, d): a copy with every matrix column-major in memory (the stand-alone entries work in place)."""
    return np.array(stack.transpose(0, 2, 1), order='C', copy=True)


# ------------------------------------------------------------------ A. k_invert
def _invert_dev(A, b, cho):
    nb, d = A.shape[:2]
    work = _colmajor(A)
    vec = None if b is None else np.array(b, order='C', copy=True)
    info = np.zeros(nb, dtype=np.int32)
    _lib.check(_lib.load().epx_invert_normal_params(0, d, nb, _lib.dptr(work), _lib.dptr(vec), int(cho),
                                                    info.ctypes.data_as(_lib.c_int32_p)))
    return work.transpose(0, 2, 1), vec, info


@pytest.mark.parametrize('cho', [False, True])
@pytest.mark.parametrize('d', dc.INVERT_DIMS)
def test_invert_batches_of_three_different_matrices(d, cho):
    for name, fams in dc.invert_batches(d):
        A, b, rows = ref = dc.invert_reference(d, name, fams, cho)
        what = 'k_invert d=%d %s cho=%d' % (d, name, cho)
        got_A, got_b, info = _invert_dev(A, b, cho)
        r = dc.invert_check(what, ref, got_A, got_b, info)
        print('%s: largest error / bound %.3e' % (what, r))
        _keep('k_invert', d, r)
        # without b: the same inverse; a member alone: the same bytes (whichever slot it had, whoever failed beside it)
        only_A, _, info2 = _invert_dev(A, None, cho)
        assert only_A.tobytes() == got_A.tobytes() and info2.tolist() == info.tolist(), what
        for i in (0, 2):
            one_A, one_b, one_info = _invert_dev(A[i:i + 1], b[i:i + 1], cho)
            assert one_A[0].tobytes() == got_A[i].tobytes() and one_b[0].tobytes() == got_b[i].tobytes(), (what, i)
        assert info.tolist() == [int(f in dc.NOT_PD) for f in fams]
    if not cho:                                                    # the Python entry on the first member of the last batch
        Q, r = util.invert_normal_params(np.asfortranarray(A[0]), b[0].copy())
        assert Q.tobytes() == np.asfortranarray(got_A[0]).tobytes() and r.tobytes() == got_b[0].tobytes()


# ------------------------------------------------------------------ B. k_olse
def _olse_dev(S, n, P):
    nb, d = S.shape[:2]
    work = _colmajor(S)
    prior = None if P is None else _colmajor(P)
    info = np.zeros(nb, dtype=np.int32)
    _lib.check(_lib.load().epx_olse(0, d, nb, _lib.dptr(work), int(n), _lib.dptr(prior), info.ctypes.data_as(_lib.c_int32_p)))
    return work.transpose(0, 2, 1), info


@pytest.mark.parametrize('with_prior', [False, True])
@pytest.mark.parametrize('d', dc.DIMS)
def test_olse_both_forms_in_batches(d, with_prior):
    for name, fams, prior in dc.olse_batches(d):
        if (prior is not None) != with_prior:
            continue
        S, P, n, rows = ref = dc.olse_reference(d, name, fams, prior)
        what = 'k_olse d=%d %s' % (d, name)
        got, info = _olse_dev(S, n, P)
        r = dc.olse_check(what, ref, got, info)                    # (the near-proportional prior: its own bound)
        print('%s: largest error / bound %.3e' % (what, r))
        _keep('k_olse', d, r)
        one, _ = _olse_dev(S[2:3], n, None if P is None else P[2:3])
        assert one[0].tobytes() == got[2].tobytes(), what
    got1 = util.olse(np.asfortranarray(S[0]), n, P=None if P is None else np.asfortranarray(P[0]))
    assert got1.tobytes() == np.asfortranarray(got[0]).tobytes()


# ------------------------------------------------------------------ C. k_moments
def _moment_records(eng, flags, sites):
    got = {}
    for k, flag in zip(sites, flags):
        scat, mean, nsamp = eng.get_tilted(k)
        dQ, dr = eng.get_site(DQI, k)
        got[k] = (mean, scat, dQ, dr, flag)
    return got


def _record_bytes(rec):
    return b''.join(np.asarray(a).tobytes() for a in rec[:4])


@pytest.mark.parametrize('d', dc.DIMS)
def test_moments_without_degrees_of_freedom(d):
    """S = d + 2: n - d - 2 = 0 and the 'sample' update is exactly -Q, -r with flag 1 (moments_check asserts it)."""
    _moment_cases_on_the_device(d, [c for c in dc.moment_cases(d) if c[0] == d + 2], False)


@pytest.mark.parametrize('est', dc.ESTIMATORS)
@pytest.mark.parametrize('d', dc.DIMS)
def test_moments_of_three_draw_sets(d, est):
    _moment_cases_on_the_device(d, [c for c in dc.moment_cases(d) if c[1] == est and c[0] != d + 2], True)


def _moment_cases_on_the_device(d, cases, first_in_depth):
    eng = engine(d, 3)
    assert cases
    for i, (S, est, fams) in enumerate(cases):
        samp, Q, r, rows = ref = dc.moments_reference(d, S, est, fams)
        what = 'k_moments d=%d S=%d (S %% 4 = %d) %s' % (d, S, S % 4, est)
        eng.set_global(Q, r)
        got = _moment_records(eng, eng.moments_batch(samp, est), range(3))
        assert eng.get_tilted(0)[2] == S
        worst = dc.moments_check(what, ref, got)
        print('%s: %s' % (what, ' '.join('%s %.2e' % kv for kv in sorted(worst.items()))))
        _keep('k_moments', d, max(worst.values()))
        if i > 0 or not first_in_depth:
            continue
        # the reversed draw order stays within the same bound
        back = _moment_records(eng, eng.moments_batch(np.asfortranarray(samp[::-1]), est), range(3))
        _keep('k_moments', d, max(dc.moments_check(what + ' reversed', ref, back).values()))
        # sites 1 and 2 alone on a fresh context: their bytes, and site 0 is left as it was
        fresh = _new_engine(d, 3)
        try:
            fresh.set_global(Q, r)
            mark_Q, mark_r = _sites(np.stack([dc.symmetric_noise(d, 200 + k) for k in range(3)])), _sites(np.stack(
                [dc.vector(d, 210 + k) for k in range(3)]))
            fresh.set_sites(DQI, mark_Q, mark_r)
            before = fresh.get_tilted(0)[:2]
            flags = fresh.moments_batch(np.asfortranarray(samp[:, :, 1:]), est, k0=1, count=2)
            part = _moment_records(fresh, flags, (1, 2))
            for k in (1, 2):
                assert _record_bytes(part[k]) == _record_bytes(got[k]) and part[k][4] == got[k][4], (what, k)
            after, (dQ0, dr0) = fresh.get_tilted(0)[:2], fresh.get_site(DQI, 0)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)), what
            assert np.array_equal(dQ0, mark_Q[:, :, 0]) and np.array_equal(dr0, mark_r[:, 0]), what
        finally:
            fresh.close()


# ------------------------------------------------------------------ D. k_cavity
def _cavities(eng, flags, sites):
    return dict((k, eng.get_cavity(k) + (flag,)) for k, flag in zip(sites, flags))


@pytest.mark.parametrize('d', dc.DIMS)
def test_cavities_of_three_sites(d):
    eng = engine(d, 3)
    for name, fams in dc.cavity_batches(d):
        Q, r, Qi, ri, rows = dc.cavity_reference(d, name, fams)
        what = 'k_cavity d=%d %s' % (d, name)
        eng.set_global(Q, r)
        eng.set_sites(QI, _sites(Qi), _sites(ri))
        got = _cavities(eng, eng.cavity_batch(QI), range(3))
        w = dc.cavity_check(what, rows, got)                       # Om == Q - Qi exactly, mu to the bound, the flags
        print('%s: largest error / bound %.3e' % (what, w))
        _keep('k_cavity', d, w)
        assert [bool(got[k][2]) for k in range(3)] == [f not in dc.NOT_PD for f in fams]
        # sites 1 and 2 alone (slot 0 and 1, sites 1 and 2) on a fresh context
        fresh = _new_engine(d, 3)
        try:
            fresh.set_global(Q, r)
            fresh.set_sites(QI, _sites(Qi), _sites(ri))
            part = _cavities(fresh, fresh.cavity_batch(QI, k0=1, count=2), (1, 2))
            for k in (1, 2):
                assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(part[k], got[k])), (what, k)
        finally:
            fresh.close()


@pytest.mark.parametrize('d', dc.DIMS)
def test_cavities_of_a_proposal(d):
    """Qi + df dQi after a trial with df = 0.37: to the bound (the compiler may contract Qi + df dQi), against the global
    approximation the device holds; that one against Q0 + sum Qi + df sum dQi."""
    df = 0.37
    eng = engine(d, 3)
    Q0, r0, Qi, ri, dQi, dri = dc.proposal_inputs(d)
    eng.set_prior(Q0, r0)
    eng.set_sites(QI, _sites(Qi), _sites(ri))
    eng.set_sites(DQI, _sites(dQi), _sites(dri))
    eng.site_sums()
    assert eng.damped_trial(df)[:2] == (True, True)
    Qg, rg = eng.get_global()
    what = 'k_cavity d=%d proposal' % d
    wide_Q = Q0.astype(LD) + Qi.astype(LD).sum(axis=0) + LD(df) * dQi.astype(LD).sum(axis=0)
    wide_r = r0.astype(LD) + ri.astype(LD).sum(axis=0) + LD(df) * dri.astype(LD).sum(axis=0)
    w = max(dc.held(what + ' global Q', Qg, Q0 + Qi.sum(axis=0) + df * dQi.sum(axis=0), wide_Q),
            dc.held(what + ' global r', rg, r0 + ri.sum(axis=0) + df * dri.sum(axis=0), wide_r))
    with np.errstate(all='ignore'):
        rows = [(dc.cavity(Qg, rg, Qi[k], ri[k], dQi[k], dri[k], df),
                 dc.cavity(Qg.astype(LD), rg.astype(LD), Qi[k], ri[k], dQi[k], dri[k], df)) for k in range(3)]
    first = _cavities(eng, [True] * 3, range(3))                  # the trial's own cavities
    got = _cavities(eng, eng.cavity_batch(QI2), range(3))
    assert all(first[k][i].tobytes() == got[k][i].tobytes() for k in range(3) for i in (0, 1))
    w = max(w, dc.cavity_check(what, rows, got, exact_Om=False))
    part = _cavities(eng, eng.cavity_batch(QI2, k0=1, count=2), (1, 2))
    assert all(part[k][i].tobytes() == got[k][i].tobytes() for k in (1, 2) for i in (0, 1))
    print('%s: largest error / bound %.3e' % (what, w))
    _keep('k_cavity(proposal)', d, w)


# ------------------------------------------------------------------ E. k_global
@pytest.mark.parametrize('d', dc.DIMS)
def test_global_moments(d):
    eng = engine(d, 3)
    for f in dc.global_families(d):
        Q, r, h, w = ref = dc.global_reference(d, f)
        eng.set_global(Q, r)
        if f in dc.NOT_PD:
            with pytest.raises(_lib.EpxError, match='not positive definite'):
                eng.global_moments()
            continue
        S, m = eng.global_moments()
        ratio = dc.global_check('k_global d=%d %s' % (d, f), ref, S, m)
        print('k_global d=%d %s: largest error / bound %.3e' % (d, f, ratio))
        _keep('k_global', d, ratio)


# ------------------------------------------------------------------ F. k_force_pd
@pytest.mark.parametrize('df', dc.DFS)
@pytest.mark.parametrize('d', dc.DIMS)
def test_force_pd_on_four_sites(d, df):
    eng = engine(d, 4)
    eps = np.finfo(np.float64).eps
    for name, thresh, fams, expected in dc.force_calls(d):
        what = 'k_force_pd d=%d %s df=%g' % (d, name, df)
        Qi, dQi = dc.force_inputs(d, fams, df)
        ri = np.stack([dc.vector(d, 150 + k) for k in range(4)])
        eng.set_sites(QI, _sites(Qi), _sites(ri))
        eng.set_sites(DQI, _sites(dQi), _sites(ri))
        forced = eng.force_pd(df, thresh, dc.TARGET)
        Qn, rn = eng.get_sites(QI)
        assert np.array_equal(rn, _sites(ri))
        ref = dc.force_reference(d, name, fams, df)
        lam_dev = [None] * 4
        for k in range(4):
            new, old = Qn[:, :, k], Qi[k]
            if not forced[k]:
                assert new.tobytes() == np.asfortranarray(old).tobytes(), (what, k, 'an unforced site was written')
                continue
            off = ~np.eye(d, dtype=bool)
            assert np.array_equal(new[off], old[off]), (what, k, 'the off-diagonal moved')
            delta = np.diag(new) - np.diag(old)
            # new_i = fl(old_i + shift): each difference new_i - old_i is the shift to 2^-53 |new_i| (and 2^-53 |shift| where the
            # subtraction rounds), so two of them agree to the sum of their roundings; the entry of smallest |new_i| says it best
            at = int(np.argmin(np.abs(np.diag(new))))
            shift = float(delta[at])
            room = 0.5 * eps * (np.abs(np.diag(new)) + abs(new[at, at]) + 2 * abs(shift))
            assert np.all(np.abs(delta - shift) <= room), (what, k, 'the diagonal did not move by one amount')
            lam_dev[k] = dc.TARGET - shift
        w = dc.force_check(what, ref, thresh, expected, lam_dev, forced)
        for k in range(4):
            if forced[k]:                                          # and the forced matrix has the target as its smallest eigenvalue
                lam, wide, norm = ref[k]
                after = Qn[:, :, k].astype(LD) + LD(df) * dQi[k].astype(LD)
                assert dc.lambda_min_within(after, dc.TARGET, dc.bound(lam, wide, norm)), (what, k)
        print('%s: largest error / bound %.3e' % (what, w))
        _keep('k_force_pd', d, w)


# ------------------------------------------------------------------ G. site sums and mix sums
def _fsum_sites(a):
    """(..., K) -> (sum over K by math.fsum, sum of the absolute values)."""
    flat = a.reshape(-1, a.shape[-1])
    return (np.array([math.fsum(row) for row in flat]), np.array([math.fsum(np.abs(row)) for row in flat]))


@pytest.mark.parametrize('K', dc.SUM_K)
@pytest.mark.parametrize('model,d', dc.SUM_MODELS)
def test_site_sums_about_the_slice_switch(model, d, K):
    eng = engine(d, K, model)
    u = 2.0 ** -53
    Q, r, dQ, dr = (np.asfortranarray(dc.mixed_values(shape, (d, K, i))) for i, shape in
                    enumerate([(d, d, K), (d, K), (d, d, K), (d, K)]))
    eng.set_sites(QI, Q, r)
    eng.set_sites(DQI, dQ, dr)
    out = eng.site_sums()
    worst, at = 0.0, 0
    for a in (Q, r, dQ, dr):
        want, mag = _fsum_sites(a.reshape((-1, K), order='F'))
        got = out[at:at + want.size]
        at += want.size
        assert np.all(np.abs(got - want) <= (K - 1) * u * mag), (model, d, K)
        if K > 1:
            worst = max(worst, float(np.max(np.abs(got - want) / ((K - 1) * u * mag))))
    assert at == out.size
    _keep('k_site_sums', d, worst)
    worst = 0.0
    # the pooled tilted moments: scatter and mean sums, and the sum of the means' outer products (one rounding per product more)
    S = d + 3
    samp = np.stack([dc.draws('mixed', S, d, 300 + k) for k in range(K)], axis=2)
    scale = dc.mixed_values((K,), (d, K, 'scale'))
    eng.set_global(dc.matrix('linear', d, 60), dc.vector(d, 61))
    eng.moments_batch(np.asfortranarray(samp * scale), 'sample')
    mix = eng.mix_sums()
    rec = [eng.get_tilted(k) for k in range(K)]
    scat = np.stack([rc[0].ravel(order='F') for rc in rec], axis=1)
    mean = np.stack([rc[1] for rc in rec], axis=1)
    d2 = d * d
    for got, a in ((mix[:d2], scat), (mix[d2:d2 + d], mean)):
        want, mag = _fsum_sites(a)
        assert np.all(np.abs(got - want) <= (K - 1) * u * mag), (model, d, K)
        if K > 1:
            worst = max(worst, float(np.max(np.abs(got - want) / np.maximum((K - 1) * u * mag, 1e-300))))
    for j in range(d):
        for i in range(d):
            prods = [Fraction(float(mean[i, k])) * Fraction(float(mean[j, k])) for k in range(K)]
            want, mag = sum(prods), sum(abs(p) for p in prods)
            err = abs(Fraction(float(mix[d2 + d + i + j * d])) - want)
            assert err <= K * Fraction(u) * mag, (model, d, K, i, j)
            worst = max(worst, float(err / (K * Fraction(u) * mag)))
    _keep('k_mix', d, worst)
    print('sums %s d=%d K=%d (nslice, per, empty = %s): largest error / bound %.3e' % (model, d, K, dc.slices(K), worst))


# ------------------------------------------------------------------ H. more workgroups than the device has L2 caches
# With ws_pointers mutated to slot 0 for every block, every batch of three above still passed.  The SUPPOSED reason (block
# placement and cache behaviour were not measured): the workgroups of a small grid go to different XCDs of an MI355X, each
# with its own L2, and do not see each other's writes to a shared slot while they run.  Seventeen blocks, more than twice the
# eight XCDs, did fail under that mutation at d = 100, 101.  Every member is held to the bytes it has in a call of its own
# (slot 0), which the tests above hold to the bound; d = 255, 256 repeat it at the largest slots, in both parities.
MANY = 17


@pytest.mark.parametrize('part', ['stand-alone', 'sites', 'force'])
@pytest.mark.parametrize('d', [100, 101, 255, 256])
def test_seventeen_blocks_keep_to_their_workspace_slots(d, part):
    assert dc.EDGES[d][2] == 'workspace' and dc.EDGES[d][3] == d | 1
    {'stand-alone': _slots_of_the_stand_alone_entries, 'sites': _slots_of_moments_and_cavities, 'force': _slots_of_force_pd}[part](d)
    _keep('workspace slots', d, 0.0)


def _slots_of_the_stand_alone_entries(d):
    A = np.stack([dc.matrix('linear', d, i) for i in range(MANY)])
    b = np.stack([dc.vector(d, 10 + i) for i in range(MANY)])
    P = np.stack([dc.matrix('linear', d, 30 + i) for i in range(MANY)])
    got_A, got_b, info = _invert_dev(A, b, False)
    got_S, info_S = _olse_dev(A, dc.olse_n(d), P)
    assert not info.any() and not info_S.any()
    for i in range(MANY):
        one_A, one_b, _ = _invert_dev(A[i:i + 1], b[i:i + 1], False)
        assert one_A[0].tobytes() == got_A[i].tobytes() and one_b[0].tobytes() == got_b[i].tobytes(), ('k_invert', d, i)
        assert _olse_dev(A[i:i + 1], dc.olse_n(d), P[i:i + 1])[0][0].tobytes() == got_S[i].tobytes(), ('k_olse', d, i)


def _slots_of_moments_and_cavities(d):
    # every site in a call of its own (k0 = k, count = 1: slot 0)
    eng = engine(d, MANY)
    Q, r = dc.matrix('linear', d, 60), dc.vector(d, 61)
    S = d + 5
    samp = np.asfortranarray(np.stack([dc.draws('mixed', S, d, 50 + k) for k in range(MANY)], axis=2))
    Qi = np.stack([4.0 * Q - dc.matrix('linear', d, 70 + k) for k in range(MANY)])
    ri = np.stack([dc.vector(d, 82 + k) for k in range(MANY)])
    eng.set_global(4.0 * Q, r)
    eng.set_sites(QI, _sites(Qi), _sites(ri))
    for est in ('sample', 'olse'):
        flags = eng.moments_batch(samp, est)
        assert flags.all()
        whole = _moment_records(eng, flags, range(MANY))
        for k in range(MANY):
            part = _moment_records(eng, eng.moments_batch(np.asfortranarray(samp[:, :, k:k + 1]), est, k0=k, count=1), (k,))
            assert _record_bytes(part[k]) == _record_bytes(whole[k]), ('k_moments', est, d, k)
    flags = eng.cavity_batch(QI)
    assert flags.all()
    whole = _cavities(eng, flags, range(MANY))
    for k in range(MANY):
        part = _cavities(eng, eng.cavity_batch(QI, k0=k, count=1), (k,))
        assert all(part[k][i].tobytes() == whole[k][i].tobytes() for i in (0, 1)), ('k_cavity', d, k)


def _slots_of_force_pd(d):
    # every site on a context of one site
    eng, one = engine(d, MANY), engine(d, 1)
    ri = np.stack([dc.vector(d, 82 + k) for k in range(MANY)])
    fams = ['linear', 'negative', 'cluster', 'diagonal'] * 5
    mats = [dc.matrix(f, d, 120 + k) for k, f in zip(range(MANY), fams)]
    dQi = np.stack([dc.symmetric_noise(d, 130 + k, 0.1) for k in range(MANY)])
    Qi = np.stack([a - 0.37 * dq for a, dq in zip(mats, dQi)])
    eng.set_sites(QI, _sites(Qi), _sites(ri))
    eng.set_sites(DQI, _sites(dQi), _sites(ri))
    forced = eng.force_pd(0.37, 1e-5, dc.TARGET)
    assert forced.tolist() == [f in ('negative', 'cluster') for f in fams[:MANY]]
    Qn = eng.get_sites(QI)[0]
    for k in range(MANY):
        one.set_sites(QI, _sites(Qi[k:k + 1]), _sites(ri[k:k + 1]))
        one.set_sites(DQI, _sites(dQi[k:k + 1]), _sites(ri[k:k + 1]))
        assert one.force_pd(0.37, 1e-5, dc.TARGET).tolist() == [forced[k]]
        assert one.get_sites(QI)[0][:, :, 0].tobytes() == np.asfortranarray(Qn[:, :, k]).tobytes(), ('k_force_pd', d, k)
