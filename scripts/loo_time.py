#!/usr/bin/env python3
"""Time one `HipEngine.loo` call at the C3 shape on the device: 512 sites of m4b_sg, D = 32, 500 rows per site, S draws
per site left by the sampler (one EP iteration through Master first; --S 800 is chains = 4, iter = 400).

What the kernel does per call: K x rows x S log-likelihoods on the matrix pipe, kept on chip, and
per row the tail selection (counting comparisons, cut short), a Zhang-Stephens fit of (30 + sqrt(M)) x M log1p, and five
passes over the row.  Down: six numbers per row.  Nothing goes up but the work list.

3 warm-up calls, then the median of `--reps`, `epx_device_synchronize` around each.  EPX_LOO_LDS_BYTES in the environment
lowers the LDS budget (fewer tiles per work item, or the workspace tile): the A/B of that choice.

    python scripts/loo_time.py [--sites 512 --D 32 --rows 500 --S 800 --reps 10] [--out FILE]
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
    ap.add_argument('--S', type=int, default=800)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    from epstan_amd import _lib, fit, loo, models
    from epstan_amd.method import Master
    if _lib.device_count() < 1:
        raise SystemExit('loo_time.py needs a HIP device: a time taken anywhere else says nothing')
    K, D = a.sites, a.D
    mod = models.m4b(K, D, a.rows)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    M = Master('m4b_sg', data.X, data.y, site_sizes=data.Nj, prior={'Q': Q0, 'r': r0}, chains=4, iter=a.S // 2,
               df0=fit.default_df0(K))
    assert M.run(1, verbose=False, calc_moments=False, seed=1) == 0
    eng = M.engine
    S = eng.num_draws()

    out = eng.loo()                                              # the right numbers, or no timing
    sl = slice(int(M.k_lim[3]), int(M.k_lim[4]))
    exp = loo.loo_host(3, D, 1, False, eng.get_draws(3, all_params=True), M.X[sl], None, M.y[sl])
    smooth = np.isfinite(exp[:, loo.LO_KHAT])
    assert np.array_equal(smooth, np.isfinite(out[sl, loo.LO_KHAT]))
    np.testing.assert_allclose(out[sl][smooth], exp[smooth], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(np.delete(out[sl], loo.LO_KHAT, axis=1), np.delete(exp, loo.LO_KHAT, axis=1), rtol=1e-8,
                               atol=1e-9)
    for _ in range(2):
        eng.loo()
    t = []
    for _ in range(a.reps):
        _lib.device_synchronize(eng.device)
        t0 = time.perf_counter()
        eng.loo()
        _lib.device_synchronize(eng.device)
        t.append(time.perf_counter() - t0)
    res = loo.summarise(out, S, M.k_lim)
    lines = [
        'loo timing: %d sites of m4b_sg, D = %d, %d rows per site, S = %d draws per site left by the sampler; '
        'EPX_LOO_LDS_BYTES = %s' % (K, D, a.rows, S, os.environ.get('EPX_LOO_LDS_BYTES', 'unset')),
        'HipEngine.loo, %d calls after 3 warm-up calls: median %.3f ms [%.3f .. %.3f]'
        % (a.reps, 1e3 * np.median(t), 1e3 * np.min(t), 1e3 * np.max(t)),
        'host copies of one call: %.1f MB down; %.2e log-likelihoods (%.2f GB as doubles)'
        % (out.nbytes / 1e6, float(out.shape[0]) * S, out.shape[0] * S * 8 / 1e9),
        'elpd_loo %.2f (se %.2f), p_loo %.2f, elpd_waic %.2f, p_waic %.2f, rows with khat above %.2f: %d of %d'
        % (res['elpd_loo'], res['se_elpd_loo'], res['p_loo'], res['elpd_waic'], res['p_waic'], res['khat_threshold'],
           res['n_bad'], out.shape[0]),
    ]
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
