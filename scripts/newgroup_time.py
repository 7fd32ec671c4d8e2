#!/usr/bin/env python3
"""Time one `Master.predict_new_group` behind a sampling launch at the C3 pool on the device: 512 sites of m4b_sg,
D = 32, 500 rows per site, 4 chains x 200 iterations (400 draws per site: a pool of N = 204 800 members at R = 1),
500 new rows in 8 new groups with responses.

One EP iteration through `Master` first.  The rows of two of the groups are compared with the NumPy statement
(newgroup.predict_new_group_host on the downloaded phi draws; a subset of the groups keeps its bits) before anything is
timed.  2 warm-up calls, then the median of `--reps` calls with `epx_device_synchronize` around each: the call's wall
time, which holds the upload of the rows, both launches, the copy-out and the one synchronisation.

    python scripts/newgroup_time.py [--sites 512 --D 32 --rows 500 --siter 200 --new-rows 500 --groups 8 --R 1 --reps 10] [--out FILE]
"""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sites', type=int, default=512)
    ap.add_argument('--D', type=int, default=32)
    ap.add_argument('--rows', type=int, default=500)
    ap.add_argument('--chains', type=int, default=4)
    ap.add_argument('--siter', type=int, default=200)
    ap.add_argument('--new-rows', type=int, default=500)
    ap.add_argument('--groups', type=int, default=8)
    ap.add_argument('--R', type=int, default=1)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from epstan_amd import _lib, fit, models, newgroup
    from epstan_amd.method import Master
    if _lib.device_count() < 1:
        raise SystemExit('newgroup_time.py needs a HIP device: a time taken anywhere else says nothing')
    K, D = a.sites, a.D
    mod = models.m4b(K, D, a.rows)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    M = Master('m4b_sg', data.X, data.y, site_sizes=data.Nj, prior={'Q': Q0, 'r': r0}, chains=a.chains, iter=a.siter,
               df0=fit.default_df0(K))
    assert M.run(1, verbose=False, calc_moments=False, seed=1) == 0
    sampling_ms = float(M.sampling_ms[-1])
    eng = M.engine
    S = eng.num_draws()
    rng = np.random.RandomState(3)
    n = a.new_rows
    Xn = rng.randn(n, D) / np.sqrt(D)
    group = rng.randint(0, a.groups, n) * 1000 + 5
    yn = (rng.rand(n) < 0.5).astype(int)

    def device():
        return M.predict_new_group(Xn, group, y_new=yn, R=a.R, seed=1)

    res = device()
    labels = res['groups'][:2]                                   # the right numbers, or no timing
    keep = np.isin(group, labels)
    phi = np.stack([np.ascontiguousarray(eng.get_draws(k)) for k in range(K)])
    rows, glpd, N = newgroup.predict_new_group_host(3, D, False, phi, Xn[keep], np.searchsorted(labels, group[keep]),
                                                    labels, yn[keep].astype(float), 1, 0, a.R)
    assert N == res['n'] == K * S * a.R
    np.testing.assert_allclose(res['f_mean'][keep], rows[:, 1], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(res['f_var'][keep] * (N - 1), rows[:, 2], rtol=1e-9)
    np.testing.assert_allclose(res['lpd'][keep], rows[:, 3], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res['group_lpd'][:2], glpd, rtol=1e-9, atol=1e-8)
    device()

    t = []
    for _ in range(a.reps):
        _lib.device_synchronize(eng.device)
        t0 = time.perf_counter()
        device()
        _lib.device_synchronize(eng.device)
        t.append((time.perf_counter() - t0) * 1e3)
    t = np.sort(t)
    lines = [
        'new-group timing: %d sites of m4b_sg, D = %d (P = %d), %d rows per site, %d chains x %d iterations, S = %d draws '
        'per site; pool of N = %d members at R = %d' % (K, D, eng.P, a.rows, a.chains, a.siter, S, N, a.R),
        'Master.predict_new_group, %d new rows in %d groups with responses, %d calls after 2 warm-up calls: median %.2f ms '
        '[%.2f .. %.2f] (wall time of the call: upload of the rows, k_newgroup over %d chunks of %d slabs, '
        'k_newgroup_merge, copy-out, one synchronisation)'
        % (n, len(res['groups']), a.reps, np.median(t), t[0], t[-1],
           -(-N // (16 * _chunk_slabs(N))), _chunk_slabs(N)),
        'sampling launch of the same EP iteration: %.1f ms; the call is %.2f %% of it'
        % (sampling_ms, 100 * np.median(t) / sampling_ms),
    ]
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


def _chunk_slabs(N):
    """newgroup_chunk_slabs of csrc/epx_kernels.h"""
    nslab = (N + 15) // 16
    return min(128, max(16, (nslab + 255) // 256))


if __name__ == '__main__':
    main()
