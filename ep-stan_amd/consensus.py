"""Consensus Monte Carlo: the `run_consensus` branch of /root/reference/experiment/fit.py:537-675.

Every site gets its own rows and the prior raised to the power 1/K, the sites are sampled independently, and the
mean and covariance of ALL sites' `phi` draws, concatenated, are the method's approximation -- repeated for a list of
iteration counts.  The sampling is K independent NUTS runs of the site densities the device serves anyway (`m*_sg`
for K == J, the multi-group programs for K < J), ONE batched launch per iteration count; the moments of the pooled
draws are taken where the draws lie (`epx_pooled_moments`, the `TODO make more efficient` of fit.py:640), two passes:
the mean first, then the scatter about it.

A `Master` built with the prior `Q0 / K`, `r0 / K` and `init_site=None` has `Qi = 0`, so the cavities it forms on
construction ARE the consensus site priors; partition, validation, sharding of the sites over the ranks and the
engine are the Master's.
"""

import os

import numpy as np

from .method import Master
from .seeds import MAX_UINT
from .util import distribute_groups

CONS_ITERS = (50, 100, 500, 1000, 2000, 4000)                 # fit.py:131
CONS_LONGER = 1.7                                             # fit.py:577: with K == J one more, longer run


def consensus_iters(K, J):
    """The iteration counts of a consensus run: CONS_ITERS and, for K == J, one run 1.7 times as long as the last
    (fit.py:575-577 appends the float `CONS_ITERS[-1]*1.7` to the module's list on EVERY call; the integer count, in a
    list of the call's own, is the evident intent)."""
    iters = list(CONS_ITERS)
    if K == J:
        iters.append(int(round(CONS_LONGER * CONS_ITERS[-1])))
    return iters


def consensus_master(model_name, model, data, conf, **master_kwargs):
    """The Master whose initial cavities are the consensus site priors (fit.py:545-599)."""
    J, K = conf.J, conf.K
    _, _, Q0, r0 = model.get_prior()
    prior = {'Q': Q0 / K, 'r': r0 / K}                                                   # fit.py:545-546
    if K < 2:
        raise ValueError("K should be at least 2.")                                      # fit.py:552-553
    if K > J:
        raise NotImplementedError("Splitting the groups not implemented.")               # fit.py:594-596
    options = dict(prior=prior, init_site=None, chains=conf.chains, warmup=None, thin=1, init='random')
    options.update(master_kwargs)
    if K < J:
        Nk, Nj_k, j_ind_k = distribute_groups(J, K, data.Nj)                             # fit.py:555-573
        return Master(model_name, data.X, data.y, A_k={'J': Nj_k}, A_n={'j_ind': j_ind_k + 1}, site_sizes=Nk, **options)
    return Master(model.site_model, data.X, data.y, site_sizes=data.Nj, **options)       # fit.py:575-592


def pooled_moments(master):
    """(m, S, n): mean and covariance (`/ (n - 1)`) of the `phi` draws of ALL sites of all ranks, concatenated, from
    the draws of the last sampling call (fit.py:639-646).  Two passes over the draws on the device: the sums give the
    mean m; the scatter about m, corrected by the sum of the residuals `x - m` of that pass, gives S.  The ranks' sums
    are added with the Master's communicator."""
    eng, comm, d = master.engine, master.comm, master.dphi
    n, s, _ = eng.pooled_moments(want_scatter=False)
    buf = comm.allreduce_sum(np.concatenate((np.asarray(s, dtype=np.float64), [float(n)])))
    n_tot = int(round(buf[d]))
    m = buf[:d] / n_tot
    n, s, sc = eng.pooled_moments(center=m)
    buf = comm.allreduce_sum(np.concatenate((np.ravel(sc, order='F'), s, [float(n)])))
    delta = buf[d * d:d * d + d] / n_tot
    S = (buf[:d * d].reshape(d, d, order='F') - n_tot * np.outer(delta, delta)) / (n_tot - 1)
    return m, S, n_tot


def run_consensus(model_name, conf, model, data, iters=None, verbose=True, **master_kwargs):
    """The consensus run of fit.py:540-675; returns the dict the reference saves as `res_c_<model>[_<id>].npz`:
    `conf, m_s_cons, S_s_cons, time_s_cons, mstepsize_s_cons, mrhat_s_cons`, one entry per iteration count
    (`iters`, default `consensus_iters(K, J)`).

    Per iteration count: one sampling launch over this rank's sites (fresh adaptation, `init='random'`, the same K
    seeds every time, as the reference starts a fresh Stan process per site), then the pooled moments.
    `mstepsize` is the mean over all sites of the sites' mean step size, `mrhat` the largest split-Rhat of any site.
    `time` is the DEVICE time of the sampling launch in seconds (max over the ranks): all sites of a rank run in one
    launch, so this is the time the whole batch took -- NOT the reference's figure, which is the Stan sampling time of
    its slowest single site (fit.py:649); the two are not the same quantity."""
    from . import fit
    J, K = conf.J, conf.K
    master = consensus_master(model_name, model, data, conf, **master_kwargs)
    iters = consensus_iters(K, J) if iters is None else [int(i) for i in iters]
    seeds = np.random.RandomState(seed=conf.seed_cons).randint(0, MAX_UINT, size=K)      # fit.py:603-606
    d = master.dphi
    eng, comm, lo, hi = master.engine, master.comm, master.k_lo, master.k_hi
    m_s_cons = np.full((len(iters), d), np.nan)                                          # fit.py:608-612
    S_s_cons = np.full((len(iters), d, d), np.nan)
    time_s_cons = np.full(len(iters), np.nan)
    mstepsize_s_cons = np.full(len(iters), np.nan)
    mrhat_s_cons = np.full(len(iters), np.nan)
    for i, it in enumerate(iters):
        if verbose:
            print('  iter {}: {}'.format(i + 1, it))
        opts = eng.sampler_opts(chains=conf.chains, iter=it, warmup=None, thin=1, init='random',
                                max_depth=master.max_treedepth, layout=master.layout)
        stats, ms = eng.sample_batch(seeds[lo:hi], opts)                                 # fit.py:622-637
        sm = comm.allreduce_sum(np.array([stats[:, 0].sum(), float(np.sum(stats[:, 7] > 0))]))
        if sm[1] > 0:                   # (every rank sees the count: none is left waiting in a collective)
            raise RuntimeError('consensus: chains of {} site(s) started at a non-finite density'.format(int(sm[1])))
        m_s_cons[i], S_s_cons[i], _ = pooled_moments(master)                             # fit.py:639-646
        mstepsize_s_cons[i] = sm[0] / K                                                  # fit.py:649-651
        mx = comm.allreduce_max(np.array([stats[:, 1].max(), ms * 1e-3]))
        mrhat_s_cons[i], time_s_cons[i] = mx[0], mx[1]
    res = dict(conf=conf.__dict__, m_s_cons=m_s_cons, S_s_cons=S_s_cons, time_s_cons=time_s_cons,
               mstepsize_s_cons=mstepsize_s_cons, mrhat_s_cons=mrhat_s_cons)
    if conf.save_res and comm.rank == 0:                                                 # fit.py:657-673
        os.makedirs(fit.RES_PATH, exist_ok=True)
        fname = 'res_c_{}_{}.npz'.format(model_name, conf.id) if conf.id else 'res_c_{}.npz'.format(model_name)
        np.savez(os.path.join(fit.RES_PATH, fname), **res)
    return res
