#!/usr/bin/env python3
"""The seed study behind SIGMA of tests/test_evidence_host.py: over `--seeds` sampler seeds, the
error LOGZ - quadrature of `evidence.site_evidence_host` on the three-parameter quadrature site (m1b_sg, D = 1, 12 rows,
cavity precision diag(4, 1)), its draws from oracle.nuts_oracle.nuts_sites, 4 chains x 400 kept draws.  Prints the
standard deviation of the error, its mean and 3 sd / sqrt(seeds), the bound the mean has to stay in; runs on the CPU.

    python scripts/evidence_study.py [--seeds 20] [--model m1b_sg]
"""

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, default=20)
    ap.add_argument('--model', default='m1b_sg')
    a = ap.parse_args()
    import test_evidence_host as t
    from epstan_amd import evidence as ev
    logq, logzk = t.quad_truth(a.model)
    err, re2, khat, its = [], [], [], []
    for seed in range(1, a.seeds + 1):
        rec, zk = t.quad_estimate(a.model, seed)
        err.append(zk - logzk)
        re2.append(rec[ev.EV_RE2])
        khat.append(rec[ev.EV_KHAT])
        its.append(rec[ev.EV_ITERS])
    err = np.array(err)
    sd = err.std(ddof=1)
    print('%s: quadrature log Z_k %.6f (log int exp(lq) %s)' % (a.model, logzk, logq))
    print('%d seeds: sd of the error %.4f, mean error %+.4f, 3 sd / sqrt(seeds) = %.4f; largest |error| %.4f'
          % (a.seeds, sd, err.mean(), 3 * sd / np.sqrt(a.seeds), np.abs(err).max()))
    print('sqrt(mean RE2) %.4f (independent draws); k-hat %.2f .. %.2f; iterations %d .. %d'
          % (np.sqrt(np.mean(re2)), min(khat), max(khat), min(its), max(its)))


if __name__ == '__main__':
    main()
