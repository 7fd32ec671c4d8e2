#!/usr/bin/env python3
"""Time `Master.mix_pred(('alpha', 'beta'))` against the host route it replaces, on the device, at the C3 shape
(512 sites of m4b_sg, D = 32, n_j = 500, 4 chains x 200 iterations: `draws` is K x 400 x 99 doubles = 162 MB).

  device route   k_named_moments over all sites (one launch, one synchronisation), K x 33 (mean, M2) records back, the
                 combination on the host
  host route     what the package offered before: Worker._save_named for every site (a device-to-host copy of the
                 site's draws and a host-side transpose each), NumPy for exp and the centred moments, the same combination

One EP iteration first (its sampler leaves the draws on the device), then warm-up calls and `--reps` timed repetitions
of each route, alternating; every call ends synchronised (the library's calls return with their stream drained), so a host
clock around it is the call's time.  The two routes' results are compared before anything is reported.  The bandwidth
line divides the bytes the kernel has to read ONCE (K S P 8; its second pass is meant to come from L2) by the time of
the whole library call -- launch, kernel, copy-back and synchronisation -- so it is a LOWER bound on the kernel's own
rate; a kernel trace (rocprofv3 --kernel-trace --stats) gives the kernel alone.

    python scripts/mix_pred_time.py [--sites 512 --D 32 --rows 500 --siter 200 --reps 7] [--out FILE]
"""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_CEILING = 6.29e12          # bytes/s, the practical copy ceiling DESIGN.md section 3 uses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sites', type=int, default=512)
    ap.add_argument('--D', type=int, default=32)
    ap.add_argument('--rows', type=int, default=500)
    ap.add_argument('--siter', type=int, default=200)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from epstan_amd import _lib, fit, models, site_params
    from epstan_amd.method import Master
    from epstan_amd.mix_pred import combine_moments
    if _lib.device_count() < 1:
        raise SystemExit('mix_pred_time.py needs a HIP device: a time taken anywhere else says nothing')
    J = K = a.sites
    mod = models.m4b(J, a.D, a.rows)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    M = Master('m4b_sg', data.X, data.y, site_sizes=data.Nj, prior={'Q': Q0, 'r': r0}, chains=4, iter=a.siter,
               df0=fit.default_df0(K))
    info = M.run(1, verbose=False, calc_moments=False, seed=1)
    assert info == 0, info
    eng = M.engine
    names = ('alpha', 'beta')
    _, shapes, hiers = mod.get_param_definitions()
    pmaps = fit._create_pmaps(hiers, J, K, None)
    S, P = eng.num_draws(), eng.P

    def device_route():
        return M.mix_pred(names, pmaps, shapes)

    def host_route():
        ns, ms, vs = [], [], []
        for w in M.workers:
            w._save_named(names)
            n = 0
            m, v = {}, {}
            for name in names:
                x = w.saved_samp[name]
                n = x.shape[0]
                m[name] = x.mean(axis=0)
                v[name] = np.square(x - m[name]).sum(axis=0)
            ns.append(n); ms.append(m); vs.append(v)
        return tuple(zip(*[combine_moments(ns, [r[p] for r in ms], [r[p] for r in vs], pmaps[i], shapes[i])
                           for i, p in enumerate(names)]))

    def kernel_call():
        return eng.named_moments(names)

    dm, dv = device_route()
    hm, hv = host_route()
    for i in range(len(names)):                 # the same numbers, or no timing
        np.testing.assert_allclose(dm[i], hm[i], rtol=1e-9)
        np.testing.assert_allclose(dv[i], hv[i], rtol=1e-9)
    kernel_call()
    t = {'device': [], 'host': [], 'call': []}
    for _ in range(a.reps):
        for key, fn in (('device', device_route), ('host', host_route), ('call', kernel_call)):
            _lib.device_synchronize(eng.device)
            t0 = time.perf_counter()
            fn()
            t[key].append(time.perf_counter() - t0)
    med = dict((k, float(np.median(v))) for k, v in t.items())
    lo = dict((k, float(np.min(v))) for k, v in t.items())
    hi = dict((k, float(np.max(v))) for k, v in t.items())
    nbytes = K * S * P * 8
    lines = [
        'mix_pred timing: %d sites of m4b_sg, D = %d, n_j = %d, 4 x %d iterations; draws %d x %d x %d doubles = %.1f MB'
        % (K, a.D, a.rows, a.siter, K, S, P, nbytes / 1e6),
        '%d repetitions of each route, alternating, after one warm-up call each; median [min .. max]' % a.reps,
        'device route  Master.mix_pred((alpha, beta))          %9.3f ms [%9.3f .. %9.3f]' % (1e3 * med['device'], 1e3 * lo['device'], 1e3 * hi['device']),
        'host route    _save_named per site + NumPy moments    %9.3f ms [%9.3f .. %9.3f]' % (1e3 * med['host'], 1e3 * lo['host'], 1e3 * hi['host']),
        'ratio host / device (medians)                         %9.1f' % (med['host'] / med['device']),
        'library call  epx_named_moments (launch + kernel + %d x %d x 2 doubles back + synchronise) %9.3f ms [%9.3f .. %9.3f]'
        % (K, 1 + a.D, 1e3 * med['call'], 1e3 * lo['call'], 1e3 * hi['call']),
        'bytes read once over the CALL time (lower bound of the kernel\'s rate) %.3f TB/s = %.1f %% of the %.2f TB/s copy ceiling'
        % (nbytes / med['call'] / 1e12, 100 * nbytes / med['call'] / HBM_COPY_CEILING, HBM_COPY_CEILING / 1e12),
        'results of the two routes agree at rtol 1e-9 (max rel. difference of the variances %.2e)'
        % max(float(np.max(np.abs(dv[i] / hv[i] - 1))) for i in range(len(names))),
    ]
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
