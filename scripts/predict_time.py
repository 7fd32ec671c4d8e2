#!/usr/bin/env python3
"""Time one `HipEngine.predict` call at the C3 shape on the device: 512 sites of m4b_sg, D = 32, 500 new rows per site,
S = 400 draws per site (`draws` is K x 400 x 99 doubles = 162 MB).

The model the figure should be near: the kernel reads each site's draws once per workgroup of 64
rows (the second pass and the other workgroups of a site come from L2) -- about 0.25 GB with the new rows -- and
evaluates 2 x K x rows x S ~ 2 x 10^8 links: a fraction of a millisecond of device work, plus the host copies of the
call (rows in, four numbers per row out).

  injected (default)  the draws are handed to every call (the test hook): the call then ALSO uploads 162 MB
  --sampled           one EP iteration through Master first; the calls read the draws its sampler left on the device

3 warm-up calls, then the median of 10, `epx_device_synchronize` around each.

    python scripts/predict_time.py [--sites 512 --D 32 --rows 500 --S 400 --reps 10 --sampled] [--out FILE]
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
    ap.add_argument('--S', type=int, default=400)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sampled', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from epstan_amd import _lib, fit, models, site_params
    from epstan_amd.engine import HipEngine
    from epstan_amd.method import Master
    if _lib.device_count() < 1:
        raise SystemExit('predict_time.py needs a HIP device: a time taken anywhere else says nothing')
    K, D = a.sites, a.D
    rng = np.random.RandomState(1)
    n = K * a.rows
    Xn = rng.randn(n, D)
    yn = (rng.rand(n) < 0.5).astype(np.float64)
    lim = np.arange(K + 1, dtype=np.int64) * a.rows
    theta = None
    if a.sampled:
        mod = models.m4b(K, D, a.rows)
        data = mod.simulate_data(Sigma_x='rand', rng=100)
        _, _, Q0, r0 = mod.get_prior()
        M = Master('m4b_sg', data.X, data.y, site_sizes=data.Nj, prior={'Q': Q0, 'r': r0}, chains=4, iter=a.S // 2,
                   df0=fit.default_df0(K))
        assert M.run(1, verbose=False, calc_moments=False, seed=1) == 0
        eng = M.engine
        S = eng.num_draws()
        check = eng.get_draws(3, all_params=True)
    else:
        X = rng.randn(K * 2, D)                                  # the context's own rows play no part
        eng = HipEngine('m4b_sg', X, (rng.rand(K * 2) < 0.5).astype(int), np.arange(K + 1) * 2)
        S = a.S
        theta = 0.5 * rng.randn(K, S, eng.P) + 0.3
        check = theta[3]

    def call():
        return eng.predict(Xn, lim, y=yn, theta=theta)

    out = call()                                                 # the right numbers, or no timing
    sl = slice(int(lim[3]), int(lim[4]))
    exp = site_params.predict_host(3, D, 1, False, check, Xn[sl], None, yn[sl])
    np.testing.assert_allclose(out[sl], exp, rtol=1e-9, atol=1e-10)
    for _ in range(2):
        call()
    t = []
    for _ in range(a.reps):
        _lib.device_synchronize(eng.device)
        t0 = time.perf_counter()
        call()
        _lib.device_synchronize(eng.device)
        t.append(time.perf_counter() - t0)
    up = (Xn.nbytes + yn.nbytes + (theta.nbytes if theta is not None else 0)) / 1e6
    lines = [
        'predict timing: %d sites of m4b_sg, D = %d, %d new rows per site, S = %d draws per site (%s); draws %.1f MB'
        % (K, D, a.rows, S, 'left by the sampler' if a.sampled else 'injected with every call', K * S * eng.P * 8 / 1e6),
        'HipEngine.predict with responses, %d calls after 3 warm-up calls: median %.3f ms [%.3f .. %.3f]'
        % (a.reps, 1e3 * np.median(t), 1e3 * np.min(t), 1e3 * np.max(t)),
        'host copies of one call: %.1f MB up, %.1f MB down; %.2e link evaluations' % (up, out.nbytes / 1e6, 2.0 * n * S),
    ]
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
