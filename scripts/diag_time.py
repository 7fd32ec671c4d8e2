#!/usr/bin/env python3
"""Time one `HipEngine.draw_diagnostics` call behind a sampling launch at the default benchmark shape on the device:
512 sites of m4b_sg, D = 32, 500 rows per site, 4 chains x 200 iterations (`draws` is K x 400 x 99 doubles = 162 MB).

The model the figure should be near: the kernel reads every site's draws once from HBM (the
later passes come from L2) and spends about 2 GFLOP of FP64 vector work on the lags -- tens of microseconds of device
work -- plus the launch, the copy-out of K x 99 x 6 doubles (2.4 MB) and one synchronisation.  It is compared with the
sampling launch of the SAME EP iteration (`Master.sampling_ms`), whose draws it describes: the call is meant to cost
less than 1 % of it.

One EP iteration through `Master` first; the result of site 3 is compared with `diagnostics_host` before anything is
timed.  3 warm-up calls, then the median of `--reps` calls with `epx_device_synchronize` around each.

    python scripts/diag_time.py [--sites 512 --D 32 --rows 500 --siter 200 --reps 20] [--out FILE]
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
        raise SystemExit('diag_time.py needs a HIP device: a time taken anywhere else says nothing')
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

    out = eng.draw_diagnostics()                                 # the right numbers, or no timing
    exp = diagnostics.diagnostics_host(np.ascontiguousarray(eng.get_draws(3, all_params=True)), a.chains)
    np.testing.assert_allclose(out[3], exp, rtol=1e-9)
    for _ in range(2):
        eng.draw_diagnostics()
    t = []
    for _ in range(a.reps):
        _lib.device_synchronize(eng.device)
        t0 = time.perf_counter()
        eng.draw_diagnostics()
        _lib.device_synchronize(eng.device)
        t.append(time.perf_counter() - t0)
    full = M.diagnostics()
    med = 1e3 * float(np.median(t))
    lines = [
        'diagnostics timing: %d sites of m4b_sg, D = %d (P = %d), %d rows per site, %d chains x %d iterations, '
        'S = %d draws per site; draws %.1f MB' % (K, D, eng.P, a.rows, a.chains, a.siter, S, K * S * eng.P * 8 / 1e6),
        'HipEngine.draw_diagnostics, %d calls after 3 warm-up calls: median %.3f ms [%.3f .. %.3f]; %.2f MB down'
        % (a.reps, med, 1e3 * np.min(t), 1e3 * np.max(t), out.nbytes / 1e6),
        'sampling launch of the same EP iteration: %.1f ms; the call is %.3f %% of it' % (sampling_ms, 100 * med / sampling_ms),
        'that iteration: largest Rhat %.3f, ESS / n of the mean: median %.2f, smallest %.3f; of the second moment: median '
        '%.2f, smallest %.3f; worst (site, coordinate) %s'
        % (np.nanmax(full['site_max_rhat']), np.nanmedian(full['ess']) / full['n'][0], np.nanmin(full['ess']) / full['n'][0],
           np.nanmedian(full['ess_sq']) / full['n'][0], np.nanmin(full['ess_sq']) / full['n'][0], full['worst']),
    ]
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
