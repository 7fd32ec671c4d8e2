#!/usr/bin/env python3
"""Every array the update stage's entries return, saved for a bit-for-bit comparison of two builds of libepx.so on one
device, and the stage's two timings.  Sites of m1b_sg (d = D + 1, three rows each) with random site parameters and
updates, fixed seeds, at d = 5, 66, 99, 100 and 130 (99 / 100: the dense kernels' work matrices leave the LDS for the global
workspace): site_sums, damped_trial, update_trial (with statistics and moments) and get_global / get_cavity behind them per
trial factor, damp_sweep, get_sites of the proposal, accept, force_pd, global_moments, cavity_batch, moments_batch with
get_tilted, mix_sums, util.invert_normal_params and util.olse.

    python scripts/update_entries_dump.py --out a.npz                    # this tree's library
    EPX_LIB=/path/to/other/libepx.so python scripts/update_entries_dump.py --out b.npz
    python scripts/update_entries_dump.py --compare a.npz b.npz          # the same bytes in every array
    python scripts/update_entries_dump.py --time                         # 512 sites, d = 66: medians in ms
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from draw_entries_dump import compare                      # noqa: E402

SHAPES = [(5, 3), (66, 6), (99, 3), (100, 3), (130, 4)]                 # d, sites
TRIALS = [0.25, 0.75, 2.0, 6.0, 20.0, -3.0]                             # passing, cavity-failing and global-failing factors
QI, QI2, DQI = 0, 1, 2


def problem(d, K, seed):
    """The engine with prior, site parameters and updates set; the target of the sweep.  (The construction of _sweep_problem in
    tests/test_gpu_parity.py, restated: the script runs without the test tree.  A change to one belongs in the other.)"""
    from epstan_amd.engine import HipEngine
    rng = np.random.RandomState(seed)

    def spd(scale):
        A = rng.randn(d, d + 5)
        return np.asfortranarray(A.dot(A.T) / (d + 5) * scale)
    Q0, r0 = spd(1.0) + np.eye(d), rng.randn(d)
    Qi = np.zeros((d, d, K), order='F'); ri = np.zeros((d, K), order='F')
    dQi = np.zeros((d, d, K), order='F'); dri = np.zeros((d, K), order='F')
    for k in range(K):
        Qi[:, :, k] = spd(0.5); ri[:, k] = rng.randn(d)
        B = rng.randn(d, d) * 0.15
        dQi[:, :, k] = spd(0.4) - 0.25 * Qi[:, :, k] + 0.5 * (B + B.T); dri[:, k] = rng.randn(d)
    X = rng.randn(K * 3, d - 1); y = (rng.rand(K * 3) < 0.5).astype(int)
    eng = HipEngine('m1b_sg', X, y, np.arange(K + 1) * 3)
    assert eng.d == d
    eng.set_prior(Q0, r0); eng.set_sites(QI, Qi, ri); eng.set_sites(DQI, dQi, dri)
    m_t = rng.randn(d) * 0.1; S_t = spd(0.2) + 0.05 * np.eye(d)
    return eng, (m_t, S_t, rng.multivariate_normal(m_t, S_t, size=64)), rng


def state(eng, tag, out):
    """What a trial leaves on the device: the global approximation and every site's cavity."""
    out[tag + '/Q'], out[tag + '/r'] = eng.get_global()
    for k in range(eng.K):
        out['%s/cav_Om/%d' % (tag, k)], out['%s/cav_mu/%d' % (tag, k)] = eng.get_cavity(k)


def entries(d, K, out):
    from epstan_amd import util
    eng, (m_t, S_t, samp), rng = problem(d, K, 100 + d)
    tag = 'd%d' % d
    sums = out[tag + '/site_sums'] = eng.site_sums()
    damps = np.concatenate((np.linspace(0, 1, 33)[1:-1], [2.0, 6.0, 20.0, -3.0]))
    for df in TRIALS:
        t = '%s/df%g' % (tag, df)
        out[t + '/damped_trial'] = np.array(eng.damped_trial(df, sums), dtype=np.int64)
        state(eng, t + '/damped', out)
        g, c, fb, ssum, smax, S, m = eng.update_trial(df, True, stat_sum=rng.randn(8), stat_max=rng.randn(8), want_moments=True)
        out[t + '/update_trial'] = np.array([g, c, fb], dtype=np.int64)
        out[t + '/stat_sum'], out[t + '/stat_max'] = ssum, smax
        if g:                                            # (S, m are not written behind a failed global check)
            out[t + '/S'], out[t + '/m'] = S, m
            out[t + '/global_moments/S'], out[t + '/global_moments/m'] = eng.global_moments()
        state(eng, t + '/update', out)
        out[t + '/update_trial_again'] = np.array(eng.update_trial(df, False)[:3], dtype=np.int64)       # (without the sums)
        out[t + '/cavity_batch_qi2'] = eng.cavity_batch(QI2)
        for which, name in ((QI, 'Qi'), (QI2, 'Qi2'), (DQI, 'dQi')):
            out['%s/sites/%s' % (t, name)], out['%s/sites/%s_r' % (t, name)] = eng.get_sites(which)
    out[tag + '/damp_sweep'] = eng.damp_sweep(damps, sums, m_t, S_t, samp)
    out[tag + '/damp_sweep_dev_sums'] = eng.damp_sweep(damps[::5], None, m_t, S_t, None)
    state(eng, tag + '/sweep', out)
    # the moment stage on injected draws, both estimators, and the mixture sums behind it
    eng.update_trial(0.25, True)
    draws = np.asfortranarray(rng.randn(2 * d + 7, d, K) * 0.5 + 0.1)
    for estim in ('sample', 'olse'):
        out['%s/moments_%s' % (tag, estim)] = eng.moments_batch(draws, estim)
        for k in range(K):
            Mat, vec, n = eng.get_tilted(k)
            out['%s/tilted_%s/%d' % (tag, estim, k)], out['%s/tilted_%s_mean/%d' % (tag, estim, k)] = Mat, vec
        out['%s/dQi_%s' % (tag, estim)], out['%s/dri_%s' % (tag, estim)] = eng.get_sites(DQI)
        out['%s/mix_sums_%s' % (tag, estim)] = eng.mix_sums()
    # accept, then the sums and cavities of the accepted sites; force_pd on an update that breaks them
    eng.update_trial(0.5, True)
    eng.accept(0.5)
    out[tag + '/accepted_Qi'], out[tag + '/accepted_ri'] = eng.get_sites(QI)
    out[tag + '/accepted_sums'] = eng.site_sums()
    out[tag + '/cavity_batch_qi'] = eng.cavity_batch(QI)
    state(eng, tag + '/accepted', out)
    dQ = np.zeros((d, d, K), order='F')
    for k in range(K):
        dQ[:, :, k] = -(1.0 + k) * np.eye(d)
    eng.set_sites(DQI, dQ, np.zeros((d, K), order='F'))
    out[tag + '/force_pd'] = eng.force_pd(0.8, 1e-5, 0.5)
    out[tag + '/forced_Qi'] = eng.get_sites(QI)[0]
    out[tag + '/forced_dQi'] = eng.get_sites(DQI)[0]
    eng.close()
    # the stand-alone operations
    A = rng.randn(d, d + 3)
    S = np.asfortranarray(A.dot(A.T) / (d + 3) + 0.1 * np.eye(d))
    out[tag + '/invert_Q'], out[tag + '/invert_r'] = util.invert_normal_params(S, rng.randn(d))
    out[tag + '/invert_cho'] = util.invert_normal_params(np.asfortranarray(np.linalg.cholesky(S).T), cho_form=True)[0]
    out[tag + '/olse'] = util.olse(S, 4 * d)
    out[tag + '/olse_prior'] = util.olse(S, 4 * d, P=np.asfortranarray(np.eye(d) * 2.0))


def dump(path):
    from epstan_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit('update_entries_dump.py needs a HIP device')
    out = {}
    for d, K in SHAPES:
        entries(d, K, out)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **{k: np.asarray(v) for k, v in out.items()})
    print('%d arrays, %d numbers -> %s (%s)' % (len(out), sum(np.size(v) for v in out.values()), path, _lib.LIB_PATH))


def timing():
    """512 sites at d = 66 (the update stage's share of the C3 shape): the median of 200 update_trial(df, True) calls and of
    20 damp_sweep calls of 31 factors, each between epx_device_synchronize, after 3 warm-up calls."""
    from epstan_amd import _lib
    eng, (m_t, S_t, samp), _ = problem(66, 512, 66)
    damps = np.linspace(0, 1, 33)[1:-1]
    sums = eng.site_sums()

    def median_ms(call, reps):
        for _ in range(3):
            call()
        ts = []
        for _ in range(reps):
            _lib.device_synchronize(0)
            t0 = time.perf_counter()
            call()
            _lib.device_synchronize(0)
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))
    trial = median_ms(lambda: eng.update_trial(0.5, True), 200)
    sweep = median_ms(lambda: eng.damp_sweep(damps, sums, m_t, S_t, samp), 20)
    eng.close()
    print(json.dumps({'lib': _lib.LIB_PATH, 'update_trial_ms': trial[0], 'update_trial_min_max_ms': trial[1:],
                      'damp_sweep_31_ms': sweep[0], 'damp_sweep_31_min_max_ms': sweep[1:]}))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--compare', nargs=2, default=None)
    ap.add_argument('--time', action='store_true')
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if a.time:
        timing()
    else:
        dump(a.out or os.path.join(ROOT, 'results', 'update_entries.npz'))
