#!/usr/bin/env python3
"""Time `Master.diagnostics(rank=True)` and plain `Master.diagnostics()` behind a sampling launch at the default benchmark
shape on the device: 512 sites of m4b_sg, D = 32, 500 rows per site, 4 chains x 200 iterations (800 used draws of 99
coordinates per site).  The figures DESIGN.md section 3.2 quotes for the kernel k_rank_diag come from here.

One EP iteration through `Master` first; the rank-normalised record of site 3 is compared with
`diagnostics.rank_diagnostics_host` before anything is timed.  3 warm-up calls of each, then the two calls alternate
`--reps` times with `epx_device_synchronize` around each; medians are reported, with the engine calls alone
(`HipEngine.draw_rank_diagnostics`, `HipEngine.draw_diagnostics`) timed the same way.

    python scripts/rank_diag_time.py [--sites 512 --D 32 --rows 500 --siter 200 --reps 20] [--out FILE]
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
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from epstan_amd import _lib, diagnostics, fit, models
    from epstan_amd.method import Master
    if _lib.device_count() < 1:
        raise SystemExit('rank_diag_time.py needs a HIP device: a time taken anywhere else says nothing')
    K, D = a.sites, a.D
    mod = models.m4b(K, D, a.rows)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    M = Master('m4b_sg', data.X, data.y, site_sizes=data.Nj, prior={'Q': Q0, 'r': r0}, chains=a.chains, iter=a.siter,
               df0=fit.default_df0(K))
    assert M.run(1, verbose=False, calc_moments=False, seed=1) == 0
    sampling_ms = float(M.sampling_ms[-1])
    eng = M.engine

    out = eng.draw_rank_diagnostics()                            # the right numbers, or no timing
    exp = diagnostics.rank_diagnostics_host(np.ascontiguousarray(eng.get_draws(3, all_params=True)), a.chains)
    np.testing.assert_allclose(out[3], exp, rtol=1e-9)

    def timed(call):
        _lib.device_synchronize(eng.device)
        t0 = time.perf_counter()
        call()
        _lib.device_synchronize(eng.device)
        return 1e3 * (time.perf_counter() - t0)

    calls = [('Master.diagnostics(rank=True)', lambda: M.diagnostics(rank=True)),
             ('Master.diagnostics()', M.diagnostics),
             ('HipEngine.draw_rank_diagnostics', eng.draw_rank_diagnostics),
             ('HipEngine.draw_diagnostics', eng.draw_diagnostics)]
    for _, call in calls:
        for _ in range(3):
            call()
    t = [[] for _ in calls]
    for _ in range(a.reps):                                      # alternating: the spread hits all four alike
        for i, (_, call) in enumerate(calls):
            t[i].append(timed(call))
    full = M.diagnostics(rank=True)
    n = int(full['n'][0])
    lines = ['rank diagnostics timing: %d sites of m4b_sg, D = %d (P = %d), %d rows per site, %d chains x %d iterations, '
             '%d used draws per site; %d workgroups of %d bytes of LDS'
             % (K, D, eng.P, a.rows, a.chains, a.siter, n, K * eng.P, 20 * n)]
    for (name, _), ti in zip(calls, t):
        lines.append('%s, %d calls after 3 warm-up calls: median %.3f ms [%.3f .. %.3f]'
                     % (name, a.reps, np.median(ti), np.min(ti), np.max(ti)))
    lines.append('sampling launch of the same EP iteration: %.1f ms; Master.diagnostics(rank=True) is %.2f %% of it'
                 % (sampling_ms, 100 * np.median(t[0]) / sampling_ms))
    lines.append('that iteration: largest rhat %.3f, largest rhat_rank %.3f (bulk %.3f, folded %.3f); ESS / n: bulk median '
                 '%.2f, smallest %.3f; tail median %.2f, smallest %.3f'
                 % (np.nanmax(full['rhat']), np.nanmax(full['rhat_rank']), np.nanmax(full['rhat_bulk']),
                    np.nanmax(full['rhat_folded']), np.nanmedian(full['ess_bulk']) / n, np.nanmin(full['ess_bulk']) / n,
                    np.nanmedian(full['ess_tail']) / n, np.nanmin(full['ess_tail']) / n))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
