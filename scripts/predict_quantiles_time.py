#!/usr/bin/env python3
"""Time `Master.predict_quantiles(scale='mean')` at the C3 shape on the device, with `Master.predict` on the same rows
beside it (the yardstick for the row-tile walk alone) and the host route it replaces (every site's draws through
`get_draws`, f and the order statistics in NumPy), forced over the same engine: 512 sites of m4b_sg, D = 32, the 500
training rows of every site as new rows, S draws per site left by the sampler (one EP iteration through Master first;
--S 800 is chains = 4, iter = 400), the default five probabilities.

What k_predict_order does per call: ONE pass of the row-tile walk over K x rows x S cells on the
matrix pipe, the cells' keys to LDS, a bitonic sort of every row there.  Up: the rows and the work list.  Down: the ten
order statistics per row the five probabilities need.

3 warm-up calls each, then `--reps` calls each, alternating, with `epx_device_synchronize` around each: median and range.
The host route is called `--host-reps` times (it takes seconds).

    python scripts/predict_quantiles_time.py [--sites 512 --D 32 --rows 500 --S 800 --reps 10 --host-reps 2] [--out FILE]
"""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _HostRoute(object):
    """Stands in for `Master._queries`: everything from the host route."""

    def __init__(self, host):
        self.host = host

    def __getattr__(self, name):
        return getattr(self.host, name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sites', type=int, default=512)
    ap.add_argument('--D', type=int, default=32)
    ap.add_argument('--rows', type=int, default=500)
    ap.add_argument('--S', type=int, default=800)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-reps', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from epstan_amd import _lib, fit, models, predict_quantiles as pq, quantiles, site_params
    from epstan_amd.method import Master
    if _lib.device_count() < 1:
        raise SystemExit('predict_quantiles_time.py needs a HIP device: a time taken anywhere else says nothing')
    K, D = a.sites, a.D
    mod = models.m4b(K, D, a.rows)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    M = Master('m4b_sg', data.X, data.y, site_sizes=data.Nj, prior={'Q': Q0, 'r': r0}, chains=4, iter=a.S // 2,
               df0=fit.default_df0(K))
    assert M.run(1, verbose=False, calc_moments=False, seed=1) == 0
    eng = M.engine
    S = eng.num_draws()
    probs = (0.025, 0.25, 0.5, 0.75, 0.975)
    ranks, plan = quantiles.rank_plan(S, probs)

    res = M.predict_quantiles(M.X, site_sizes=M.Nk)              # the right numbers, or no timing
    sl = slice(int(M.k_lim[3]), int(M.k_lim[4]))
    f = site_params.linear_predictor(3, D, 1, False, eng.get_draws(3, all_params=True), M.X[sl], None)
    np.testing.assert_allclose(res['quantiles'][:, sl], np.quantile(pq.stable_sigmoid(f), probs, axis=0), rtol=1e-9)

    def timed(call):
        _lib.device_synchronize(eng.device)
        t0 = time.perf_counter()
        call()
        _lib.device_synchronize(eng.device)
        return time.perf_counter() - t0

    def host_route():
        resolver = M._queries
        M._queries = _HostRoute(resolver.host)
        try:
            return M.predict_quantiles(M.X, site_sizes=M.Nk)
        finally:
            M._queries = resolver

    calls = {'Master.predict_quantiles': lambda: M.predict_quantiles(M.X, site_sizes=M.Nk),
             'Master.predict': lambda: M.predict(M.X, site_sizes=M.Nk),
             'HipEngine.predict_order_stats': lambda: eng.predict_order_stats(M.X, M.k_lim, ranks),
             'HipEngine.predict': lambda: eng.predict(M.X, M.k_lim)}
    for call in calls.values():
        for _ in range(3):
            call()
    t = dict((name, []) for name in calls)
    for _ in range(a.reps):
        for name, call in calls.items():
            t[name].append(timed(call))
    host = host_route()
    err = np.abs(host['quantiles'] - res['quantiles']).max()
    th = [timed(host_route) for _ in range(a.host_reps)]
    lines = ['predict_quantiles timing: %d sites of m4b_sg, D = %d, %d rows per site as new rows, S = %d draws per site left by '
             'the sampler, %d order statistics per row; library %s' % (K, D, a.rows, S, ranks.size,
                                                                        os.environ.get('EPX_LIB', 'as built'))]
    for name in calls:
        lines.append('%-30s %d calls after 3 warm-up calls: median %.3f ms [%.3f .. %.3f]'
                     % (name, a.reps, 1e3 * np.median(t[name]), 1e3 * np.min(t[name]), 1e3 * np.max(t[name])))
    lines.append('%-30s %d calls after 1: median %.1f ms [%.1f .. %.1f]; largest |host - device| quantile %.3e'
                 % ('host route (get_draws, NumPy)', a.host_reps, 1e3 * np.median(th), 1e3 * np.min(th), 1e3 * np.max(th), err))
    mq, mp = np.median(t['Master.predict_quantiles']), np.median(t['Master.predict'])
    lines.append('Master.predict_quantiles / Master.predict: %.2f;  host route / Master.predict_quantiles: %.1f;  '
                 'HipEngine.predict_order_stats / HipEngine.predict: %.2f'
                 % (mq / mp, np.median(th) / mq, np.median(t['HipEngine.predict_order_stats']) / np.median(t['HipEngine.predict'])))
    lines.append('%.2e cells; %.1f MB of rows up, %.1f MB of order statistics down; the host route downloads %.1f MB of draws'
                 % (float(M.N) * S, M.X.nbytes / 1e6, M.N * ranks.size * 8 / 1e6, K * S * eng.P * 8 / 1e6))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
