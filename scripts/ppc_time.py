#!/usr/bin/env python3
"""Time `Master.ppc()` at the C3 shape on the device, `Master.loo()` beside it in the same process: 512 sites of m4b_sg,
D = 32, 500 rows per site, S draws per site left by the sampler (one EP iteration through Master first; --S 800 is
chains = 4, iter = 400).

What k_ppc does per call: ONE pass of the row-tile walk over K x rows x S cells on the matrix
pipe, one Philox call and two log-likelihoods per cell, the rows added up per draw on chip.  Down: eight numbers per
group and per site.  Nothing goes up but the work list.

3 warm-up calls each, then `--reps` calls each, alternating, with `epx_device_synchronize` around each: median and range.
EPX_LIB in the environment names another build of the library (make variant ... EXTRA=-DEPX_PPC_WAVES=1: the A/B of the
kernel's register cap).

    python scripts/ppc_time.py [--sites 512 --D 32 --rows 500 --S 800 --reps 10] [--out FILE]
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

    from epstan_amd import _lib, fit, models, ppc
    from epstan_amd.method import Master
    if _lib.device_count() < 1:
        raise SystemExit('ppc_time.py needs a HIP device: a time taken anywhere else says nothing')
    K, D = a.sites, a.D
    mod = models.m4b(K, D, a.rows)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    M = Master('m4b_sg', data.X, data.y, site_sizes=data.Nj, prior={'Q': Q0, 'r': r0}, chains=4, iter=a.S // 2,
               df0=fit.default_df0(K))
    assert M.run(1, verbose=False, calc_moments=False, seed=1) == 0
    eng = M.engine
    S = eng.num_draws()

    res = M.ppc(seed=1)                                          # the right numbers, or no timing
    sl = slice(int(M.k_lim[3]), int(M.k_lim[4]))
    groups, sites, _ = ppc.ppc_host(3, D, [1], False, [eng.get_draws(3, all_params=True)], M.X[sl], None, M.y[sl],
                                    np.array([0, sl.stop - sl.start]), seed=1, row0=sl.start)
    exp = ppc.summarise(groups, sites, S, [1])
    for key in ('t_obs', 't_rep_mean', 'p_t_ge', 'p_t', 'p_d'):
        assert res[key][3] == exp[key][0], key
    np.testing.assert_allclose([res['d_obs_mean'][3], res['d_rep_mean'][3]], [exp['d_obs_mean'][0], exp['d_rep_mean'][0]],
                               rtol=1e-9)

    def timed(call):
        _lib.device_synchronize(eng.device)
        t0 = time.perf_counter()
        call()
        _lib.device_synchronize(eng.device)
        return time.perf_counter() - t0

    calls = {'Master.ppc': lambda: M.ppc(seed=1), 'Master.loo': M.loo,
             'HipEngine.replicated_checks': lambda: eng.replicated_checks(seed=1), 'HipEngine.loo': eng.loo}
    for call in calls.values():
        for _ in range(3):
            call()
    t = dict((name, []) for name in calls)
    for _ in range(a.reps):
        for name, call in calls.items():
            t[name].append(timed(call))
    lines = ['ppc timing: %d sites of m4b_sg, D = %d, %d rows per site, S = %d draws per site left by the sampler; library %s'
             % (K, D, a.rows, S, os.environ.get('EPX_LIB', 'as built'))]
    for name in calls:
        lines.append('%-28s %d calls after 3 warm-up calls: median %.3f ms [%.3f .. %.3f]'
                     % (name, a.reps, 1e3 * np.median(t[name]), 1e3 * np.min(t[name]), 1e3 * np.max(t[name])))
    lines.append('Master.ppc / Master.loo: %.3f;  HipEngine.replicated_checks / HipEngine.loo: %.3f'
                 % (np.median(t['Master.ppc']) / np.median(t['Master.loo']),
                    np.median(t['HipEngine.replicated_checks']) / np.median(t['HipEngine.loo'])))
    lines.append('%.2e cells; groups outside [%.3f, %.3f]: %d of %d; mean p_t %.3f, mean p_d %.3f'
                 % (float(M.N) * S, res['level'] / 2, 1 - res['level'] / 2, res['extreme'].size, res['p_t'].size,
                    res['p_t'].mean(), res['p_d'].mean()))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
