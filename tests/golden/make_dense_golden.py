"""Writes tests/golden/dense_edge_lambda.npz: the longdouble lambda_min (tests/dense_edge_cases.py: lambda_min, by bisection
on the inertia from Gershgorin's bounds, no bracket) of every force-pd site of the case table at d >= GOLDEN_FROM, each as
the two doubles whose sum it is.  The matrices are not stored: the table regenerates them from its seeds.

    python tests/golden/make_dense_golden.py
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import dense_edge_cases as dc                                    # noqa: E402


def main():
    out = {}
    for d in dc.DIMS:
        if d < dc.GOLDEN_FROM:
            continue
        for name, _, fams, _ in dc.force_calls(d):
            for df in dc.DFS:
                A = dc.force_matrices(d, fams, df, np.longdouble)
                for k in range(len(fams)):
                    lam = dc.lambda_min(A[k])
                    hi = np.float64(lam)
                    out[dc.golden_key(d, name, df, k)] = np.array([hi, np.float64(lam - np.longdouble(hi))])
                    print(dc.golden_key(d, name, df, k), repr(lam), flush=True)
    np.savez(dc.GOLDEN, **out)


if __name__ == '__main__':
    main()
