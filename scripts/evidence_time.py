#!/usr/bin/env python3
"""Time `epx_site_evidence` at the C3 shape on the device, `Master.loo()` beside it in the same process: 512 sites of
m4b_sg, D = 32, 500 rows per site, 4 chains x 200 iterations (S = 400 draws per site left by the sampler, N1 = 200: the
fit set's 200 draws are just the 2 P = 198 the proposal needs); one EP iteration through Master first.

What the three kernels do per call: per site a 99 x 99 scatter on the matrix pipe and its packed
Cholesky factor in LDS; 2 N1 columns of forward substitutions or proposal draws, cavity forms and ONE pass of the row-tile
walk over rows x 2 N1 cells; a few bridge iterations over 2 N1 terms in LDS.  Down: six numbers per site.

`epx_site_evidence`: its own device time (elapsed_ms, events around the three launches), 2 warm-up calls, then the median
of `--reps` calls.  `Master.loo` and `Master.log_evidence` (sampling launch included): host clock around a device
synchronise, the same warm-up and repetitions.

    python scripts/evidence_time.py [--sites 512 --D 32 --rows 500 --iter 200 --reps 5] [--out FILE]
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
    ap.add_argument('--iter', type=int, default=200)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from epstan_amd import _lib, evidence as ev, fit, models
    from epstan_amd.method import Master
    if _lib.device_count() < 1:
        raise SystemExit('evidence_time.py needs a HIP device: a time taken anywhere else says nothing')
    K, D = a.sites, a.D
    mod = models.m4b(K, D, a.rows)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    M = Master('m4b_sg', data.X, data.y, site_sizes=data.Nj, prior={'Q': Q0, 'r': r0}, chains=4, iter=a.iter,
               df0=fit.default_df0(K))
    assert M.run(1, verbose=False, calc_moments=False, seed=1) == 0
    eng = M.engine
    S = eng.num_draws()

    res = M.log_evidence(seed=1)                                 # the right numbers, or no timing
    out = eng.site_evidence(seed=1, site0=0)[0]
    sl = slice(int(M.k_lim[3]), int(M.k_lim[4]))
    Om, mu = eng.get_cavity(3)
    rec = ev.site_evidence_host(3, D, False, M.X[sl], M.y[sl], None, mu, Om,
                                np.ascontiguousarray(eng.get_draws(3, all_params=True)), 4, 1, 3)[0]
    np.testing.assert_allclose(out[3, [ev.EV_LOGZ, ev.EV_LOGZ_IS, ev.EV_RE2]], rec[[ev.EV_LOGZ, ev.EV_LOGZ_IS, ev.EV_RE2]],
                               rtol=1e-8)
    assert out[3, ev.EV_ITERS] == rec[ev.EV_ITERS]

    def timed(call):
        _lib.device_synchronize(eng.device)
        t0 = time.perf_counter()
        call()
        _lib.device_synchronize(eng.device)
        return 1e3 * (time.perf_counter() - t0)

    calls = {'epx_site_evidence (elapsed_ms)': lambda: eng.site_evidence(seed=1, site0=0)[2],
             'HipEngine.site_evidence (host clock)': lambda: timed(lambda: eng.site_evidence(seed=1, site0=0)),
             'Master.loo': lambda: timed(M.loo),
             'Master.log_evidence (with its sampling launch)': lambda: timed(lambda: M.log_evidence(seed=1))}
    t = {}
    for name, call in calls.items():
        for _ in range(2):
            call()
        t[name] = [call() for _ in range(a.reps)]
    lines = ['evidence timing: %d sites of m4b_sg, D = %d, %d rows per site, S = %d draws per site (N1 = %d), P = %d; library %s'
             % (K, D, a.rows, S, out[0, ev.EV_N1], eng.P, os.environ.get('EPX_LIB', 'as built'))]
    for name in calls:
        lines.append('%-48s %d calls after 2 warm-up calls: median %.3f ms [%.3f .. %.3f]'
                     % (name, a.reps, np.median(t[name]), np.min(t[name]), np.max(t[name])))
    lines.append('epx_site_evidence / Master.loo: %.3f' % (np.median(t['epx_site_evidence (elapsed_ms)'])
                                                            / np.median(t['Master.loo'])))
    lines.append('log_evidence %.3f; n_bad %d; iterations %d .. %d; sqrt(re2) median %.4f, max %.4f; k-hat median %.2f, '
                 '%d of %d above 0.7' % (res['log_evidence'], res['n_bad'], res['iters'].min(), res['iters'].max(),
                                         np.sqrt(np.median(res['re2'])), np.sqrt(np.max(res['re2'])), np.median(res['khat']),
                                         int(np.sum(res['khat'] > 0.7)), K))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
