#!/usr/bin/env python3
"""Does reusing the tilted draws across EP iterations pay?  (`Master.run(reuse=True)`, reweight.py)

Two experiments, each run twice from the same seed, without and with `reuse=True` (the default policy of
`reweight.reuse_ok`: k-hat <= loo.khat_threshold(S), WESS >= S / 2, for EVERY site of the rank):
  - `fit`: fit.py's default experiment (m4b, J = 64 groups on K = 32 sites, D = 16, 20 rows per group, 4 x 200 NUTS
    iterations per site update);
  - `c3`: the benchmark's shape (512 sites of m4b_sg, D = 32, 500 rows per site, 4 x 200).
Per iteration of the reusing run: whether it reused, how many sites passed, the largest smoothed k-hat, the smallest
WESS / S, the reweighting kernel's ms beside the sampling ms of the last sampled iteration; then the share of iterations
that qualified, the device time both runs spent in the tilted stage, and fit.kl_mvn between the two runs' final
approximations (plain || reuse), beside the same KL between two plain runs from different seeds as the scale of the
Monte-Carlo noise.

    python scripts/reuse_study.py [--which fit c3] [--iters-fit 40] [--iters-c3 12] [--out FILE]
"""

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def masters(which):
    from epstan_amd import fit, models
    from epstan_amd.method import Master
    if which == 'fit':
        return lambda: fit.main('m4b', fit.configurations(run_ep=True, save_res=False), ret_master=True, verbose=False)
    mod = models.m4b(512, 32, 500)
    data = mod.simulate_data(Sigma_x='rand', rng=100)
    _, _, Q0, r0 = mod.get_prior()
    return lambda: Master('m4b_sg', data.X, data.y, site_sizes=data.Nj, prior={'Q': Q0, 'r': r0}, chains=4, iter=200,
                          df0=models.default_df0(512))


def study(which, niter, seed=1):
    from epstan_amd import fit
    make = masters(which)
    runs = {}
    for name, kw in (('plain', dict(seed=seed)), ('reuse', dict(seed=seed, reuse=True)), ('other seed', dict(seed=seed + 1))):
        M = make()
        info, _, (stimes, _, _, _) = M.run(niter, verbose=False, return_analytics=True, **kw)
        if info:
            raise SystemExit('%s: the %s run ended with code %d' % (which, name, info))
        S, m = M.cur_approx()
        runs[name] = dict(S=S, m=m, tilted_s=float(stimes.sum()), sampling_ms=list(M.sampling_ms), log=list(M.reuse_log),
                          draws=M.engine.num_draws(), sites=M.K)
        M.engine.close()
    r = runs['reuse']
    lines = ['reuse study `%s`: %d sites, S = %d draws per site, %d EP iterations, seed %d' % (which, r['sites'], r['draws'], niter, seed),
             'iter reused n_ok/%d  khat_max  wess_min/S  reweight ms  last sampling ms' % r['sites']]
    last_ms, at = float('nan'), 0
    for i, e in enumerate(r['log']):
        if not e['reused']:
            last_ms = r['sampling_ms'][at]
            at += 1
        lines.append('%4d %6s %7d  %8.3f  %10.3f  %11.3f  %16.1f' % (i + 1, 'yes' if e['reused'] else 'no', e['n_ok'], e['khat_max'],
                                                                     e['wess_min_frac'], e['ms'], last_ms))
    n_reused = sum(e['reused'] for e in r['log'])
    lines.append('iterations that qualified: %d of %d (%.0f %% of those that could: the first always samples)'
                 % (n_reused, niter, 100.0 * n_reused / max(niter - 1, 1)))
    lines.append('device time in the tilted stage: plain %.3f s, reuse %.3f s' % (runs['plain']['tilted_s'], r['tilted_s']))
    p, o = runs['plain'], runs['other seed']
    lines.append('KL(plain || reuse) of the final approximations %.4g; KL(plain || plain from another seed) %.4g'
                 % (fit.kl_mvn(p['m'], p['S'], r['m'], r['S']), fit.kl_mvn(p['m'], p['S'], o['m'], o['S'])))
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--which', nargs='+', default=['fit', 'c3'], choices=['fit', 'c3'])
    ap.add_argument('--iters-fit', type=int, default=40)
    ap.add_argument('--iters-c3', type=int, default=12)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from epstan_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit('reuse_study.py needs a HIP device')
    for which in a.which:
        text = study(which, a.iters_fit if which == 'fit' else a.iters_c3)
        print(text, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(text + '\n\n')


if __name__ == '__main__':
    main()
