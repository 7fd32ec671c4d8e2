#!/usr/bin/env python3
"""Time one `Master.mix_quantiles(['phi', 'alpha', 'beta'])` behind a sampling launch at the C3 shape on the device:
512 sites of m4b_sg, D = 32, 500 rows per site, 4 chains x 400 iterations (800 draws per site: `draws` is
K x 800 x 99 doubles = 324 MB), against the host route in the same process: `get_draws` of every site, the models'
`transformed parameters` through site_params.named_draws, np.quantile.

`phi` is pooled over the sites (eight counting passes of k_pooled_count over all draws), `alpha` and `beta` are every
site's own (k_site_order_stats: one workgroup per (site, element) sorts 800 keys, padded to 1024, in LDS).  Only order
statistics leave the device: 512 x 99 x 10 doubles for the two mapped names, 66 x 10 x 256 counts per pass for phi.

One EP iteration through `Master` first; both routes are compared before anything is timed.  2 warm-up calls, then the
median of `--reps` calls with `epx_device_synchronize` around each; the host route is timed `--host-reps` times.

    python scripts/quantiles_time.py [--sites 512 --D 32 --rows 500 --siter 400 --reps 10 --host-reps 3] [--out FILE]
"""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sites', type=int, default=512)
    ap.add_argument('--D', type=int, default=32)
    ap.add_argument('--rows', type=int, default=500)
    ap.add_argument('--chains', type=int, default=4)
    ap.add_argument('--siter', type=int, default=400)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from epstan_amd import _lib, fit, models, site_params
    from epstan_amd.method import Master
    if _lib.device_count() < 1:
        raise SystemExit('quantiles_time.py needs a HIP device: a time taken anywhere else says nothing')
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
    pnames, pshapes, phiers = mod.get_param_definitions()
    pmaps = fit._create_pmaps(phiers, K, K, None)
    names = ['phi'] + list(pnames)
    smap, shapes = [None] + list(pmaps), [None] + list(pshapes)

    def device():
        return M.mix_quantiles(names, PROBS, smap, shapes)

    def host():
        draws = [site_params.named_draws(3, D, 1, False, True, eng.get_draws(k, all_params=True), names) for k in range(K)]
        out = [np.quantile(np.concatenate([d['phi'] for d in draws]), PROBS, axis=0, method='linear')]
        for name in pnames:
            out.append(np.moveaxis(np.stack([np.quantile(d[name], PROBS, axis=0, method='linear') for d in draws]), 0, 1))
        return out

    got, want = device(), host()                                 # the right numbers, or no timing
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        np.testing.assert_allclose(g, w, rtol=1e-9, atol=1e-12 * np.abs(w).max(), err_msg=name)
    device()

    def timed(fn):
        t = []
        for _ in range(a.reps):
            _lib.device_synchronize(eng.device)
            t0 = time.perf_counter()
            fn()
            _lib.device_synchronize(eng.device)
            t.append(time.perf_counter() - t0)
        return t
    t = timed(device)
    t_pool = timed(lambda: M.mix_quantiles('phi', PROBS))
    t_site = timed(lambda: M.mix_quantiles(list(pnames), PROBS, list(pmaps), list(pshapes)))
    ranks = np.arange(10, dtype=np.int64) * (S // 10)
    t_kern = timed(lambda: eng.named_order_stats(list(pnames), ranks))
    th = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        host()
        th.append(time.perf_counter() - t0)
    med, medh = 1e3 * float(np.median(t)), 1e3 * float(np.median(th))
    lines = [
        'quantiles timing: %d sites of m4b_sg, D = %d (P = %d), %d rows per site, %d chains x %d iterations, '
        'S = %d draws per site; draws %.1f MB' % (K, D, eng.P, a.rows, a.chains, a.siter, S, K * S * eng.P * 8 / 1e6),
        "Master.mix_quantiles(['phi', 'alpha', 'beta']), 5 probabilities (phi pooled, alpha and beta per site), %d calls after 2 "
        'warm-up calls: median %.1f ms [%.1f .. %.1f]' % (a.reps, med, 1e3 * np.min(t), 1e3 * np.max(t)),
        'of which phi alone (eight counting passes over the pool of %d draws x %d elements): median %.1f ms; alpha and beta alone '
        '(%d workgroups, each sorting %d keys): median %.1f ms, of which HipEngine.named_order_stats (launch, copy-out, the split '
        'into per-site arrays): median %.1f ms' % (K * S, eng.d, 1e3 * float(np.median(t_pool)), K * (1 + D), S,
                                                   1e3 * float(np.median(t_site)), 1e3 * float(np.median(t_kern))),
        'host route in the same process (get_draws of every site, site_params.named_draws, np.quantile), %d calls: median '
        '%.1f ms [%.1f .. %.1f]; the device route is %.1f x faster' % (a.host_reps, medh, 1e3 * np.min(th), 1e3 * np.max(th),
                                                                      medh / med),
        'sampling launch of the same EP iteration: %.1f ms; the call is %.2f %% of it' % (sampling_ms, 100 * med / sampling_ms),
    ]
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
