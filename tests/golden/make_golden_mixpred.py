#!/usr/bin/env python3
"""Generate tests/golden/mix_pred.npz by calling the reference's own `Master.mix_pred`.

Run in the build container only (needs /root/reference; CPU only):

    python tests/golden/make_golden_mixpred.py

The reference is imported as tests/golden/make_golden.py does (temporary copy, stub `pystan`).  Its
`mix_pred` (method.py:1304-1478) reads nothing of a Master but `iter` and `workers[k].fit`, and of a
fit `extract(pars=...)`, `par_dims` and `model_pars`: a bare Master whose workers carry stand-in fit
objects with known draws is all it needs.  The maps come from the reference's `_create_pmaps`
(experiment/fit.py:763-849), the parameter definitions from models/m1b.py, m4b.py.

Only data is written: per-site draws in, means and variances out.  K = 4 sites, S = 24 draws each.
"""

import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

K, S, D = 4, 24, 3


class StandInFit(object):
    """What mix_pred asks of a PyStan fit."""

    def __init__(self, draws):
        self._draws = draws
        self.model_pars = list(draws)
        self.par_dims = [list(v.shape[1:]) for v in draws.values()]

    def extract(self, pars=None):
        return {pars: self._draws[pars].copy()}          # (mix_pred centres the array it gets in place)


def bare_master(method, site_draws):
    M = object.__new__(method.Master)
    M.iter = 1
    M.workers = []
    for draws in site_draws:
        w = object.__new__(method.Worker)
        w.fit = StandInFit(draws)
        M.workers.append(w)
    return M


def draws_of(rng, shape):
    """(S,) + shape draws; every element with its own location and scale, |mean| <= 10 sd."""
    sd = np.exp(0.5 * rng.randn(*shape))
    loc = sd * rng.uniform(-10.0, 10.0, size=shape)
    return loc + sd * rng.randn(S, *shape)


def record(out, tag, names, site_draws, means, variances):
    for name, m, v in zip(names, means, variances):
        out['%s_m_%s' % (tag, name)] = np.asarray(m)
        out['%s_v_%s' % (tag, name)] = np.asarray(v)
        for k, dr in enumerate(site_draws):
            out['%s_draws_%s_%d' % (tag, name, k)] = dr[name]


def main():
    util, method, tmp = import_reference()
    try:
        import fit as ref_fit                                # /root/reference/experiment/fit.py
        from models import m1b, m4b
        rng = np.random.RandomState(20)
        out = {}

        # (i) a vector every site shares: smap None
        sd = [{'beta': draws_of(rng, (D,))} for _ in range(K)]
        m, v = bare_master(method, sd).mix_pred('beta')
        record(out, 'i', ['beta'], sd, [m], [v])

        # (ii) K == J: one group per site, the single-group programs' `real alpha`, `vector[D] beta`
        pmaps = ref_fit._create_pmaps((0, 0), K, K, None)
        sd = [{'alpha': draws_of(rng, ()), 'beta': draws_of(rng, (D,))} for _ in range(K)]
        ms, vs = bare_master(method, sd).mix_pred(['alpha', 'beta'], pmaps, [(K,), (K, D)])
        record(out, 'ii', ['alpha', 'beta'], sd, ms, vs)

        # (iii) K < J: unequal groups per site, slice maps
        Ns = np.array([2, 1, 3, 1])
        J = int(Ns.sum())
        pmaps = ref_fit._create_pmaps((0, 0), J, K, Ns)
        sd = [{'alpha': draws_of(rng, (n,)), 'beta': draws_of(rng, (n, D))} for n in Ns]
        ms, vs = bare_master(method, sd).mix_pred(['alpha', 'beta'], pmaps, [(J,), (J, D)])
        record(out, 'iii', ['alpha', 'beta'], sd, ms, vs)
        out['iii_Ns'] = Ns

        # (iv) overlapping maps: indexes 1 and 4 get two contributions, the others one (no site of length 1: the
        # reference adds an axis to those, method.py:1421-1424, which its mixed branch cannot broadcast)
        lims = np.array([[0, 2], [1, 3], [3, 5], [4, 6]])
        smap = [slice(int(a), int(b)) for a, b in lims]
        sd = [{'alpha': draws_of(rng, (int(b - a),))} for a, b in lims]
        m, v = bare_master(method, sd).mix_pred('alpha', smap, (6,))
        record(out, 'iv', ['alpha'], sd, [m], [v])
        out['iv_lims'] = lims

        # parameter definitions as plain lists
        for name, mod in (('m1b', m1b), ('m4b', m4b)):
            names, shapes, hiers = mod.model(5, D, 10).get_param_definitions()
            out['defs_' + name] = np.array(json.dumps(
                [list(names), [list(int(x) for x in s) for s in shapes], list(hiers)]))
        path = os.path.join(HERE, 'mix_pred.npz')
        np.savez_compressed(path, **out)
        print('mix_pred.npz', os.path.getsize(path), 'bytes')
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
