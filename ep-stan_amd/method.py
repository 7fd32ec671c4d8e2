"""Distributed EP driver with the API of /root/reference/epstan/method.py.

`Master` and `Worker` keep the reference's constructor arguments, public
attributes (`S m Q r Qi ri Qi2 ri2 dQi dri Q0 r0 K workers iter`, Fortran-ordered
`(d,d,K)` site arrays), methods (`run`, `cur_approx`, `Worker.cavity`,
`Worker.tilted`), return codes and error behaviour (method.py:121-1247), but
every numerical step runs on the GPU through libepx.so:

  reference (CPU)                                   here (MI355X)
  ------------------------------------------------  ------------------------------------
  for k: Worker.tilted -> Stan subprocess (:1005)   ONE batched NUTS kernel over all sites
  mean / dgeqrf / potri per site (:413-437)         batched scatter(MFMA f64)+Cholesky kernel
  Qi2 = Qi + df dQi ; Q = sum_k Qi2 + Q0 (:1071)    site sums once per iteration (affine in df)
                                                    + one RCCL all-reduce across GPUs
  cho_factor(Q) (:1080), for k: Worker.cavity       one small kernel + one batched cavity kernel,
  invert_normal_params(cho_Q, r) (:1215)            queued behind the all-reduce, one host sync

The host mirrors (`master.Qi` ...) are refreshed when `run` returns; inside `run`
the device copies are authoritative.  Sites are sharded contiguously over the
ranks of an optional communicator (`comm=dist.EpxComm()`: RCCL inside libepx.so).
"""

__all__ = ['Worker', 'Master']

import os
import sys
import time
from collections import namedtuple

import numpy as np
from numpy.linalg import LinAlgError

from . import diagnostics as _diagnostics
from . import dispatch as _dispatch
from . import dist as _dist
from . import draw_queries as _dq
from . import engine as _engine
from . import evidence as _evidence
from . import loo as _loo
from . import newgroup as _newgroup
from . import ppc as _ppc
from . import predict_quantiles as _predict_quantiles
from . import quantiles as _quantiles
from . import reweight as _reweight
from . import site_params as _site_params
from .seeds import MAX_UINT, run_seeds, stan_seed, stan_seeds
from .util import invert_normal_params


def _model_name(site_model):
    """'.../m4b_sg', 'm4b_sg.stan' or 'm4b_sg.pkl' -> 'm4b_sg' (util.load_stan
    accepts all three spellings, util.py:642-689)."""
    if not isinstance(site_model, str):
        raise TypeError('site_model has to be a path/name string selecting a built-in '
                        'GPU site model (StanModel instances cannot run on the GPU)')
    base = os.path.basename(site_model)
    for ext in ('.stan', '.pkl'):
        if base.endswith(ext):
            base = base[:-len(ext)]
    return base


def _sort_keywords(given, tables, unknown):
    """Distribute keyword arguments over option tables.

    `tables` is a sequence of dicts of defaults; returns one dict per table holding the
    table's keys with the given value or the default.  A keyword that no table knows raises
    TypeError with the message `unknown` (formatted with the keyword)."""
    known = set()
    for table in tables:
        known.update(table)
    for kw in given:
        if kw not in known:
            raise TypeError(unknown.format(kw))
    return [dict((kw, given.get(kw, default)) for kw, default in table.items()) for table in tables]


class Worker(object):
    """Per-site state and the per-site entry points `cavity` / `tilted`.

    Same constructor and attributes as the reference's Worker
    (method.py:121-265).  `Mat`/`vec` hold the cavity precision / MEAN after
    `cavity` (phase 1) and the unnormalised scatter matrix / tilted mean after
    `tilted` (phase 2); they are fetched from the device on access.

    `last_time` is the device time of the sampling launch the site took part in: inside
    `Master.run` all sites of a rank are sampled by ONE launch, so every worker of the rank
    reports the same value (the reference reports each site's own Stan time; their maximum,
    which is what `run` records in `stimes`, has the same meaning in both).
    """

    DEFAULT_OPTIONS = {
        'init_prev'       : True,
        'prec_estim'      : 'sample',
        'prec_estim_skip' : 0,
        'verbose'         : False
    }

    DEFAULT_STAN_PARAMS = {
        'chains'          : 4,
        'iter'            : 1000,
        'warmup'          : None,
        'thin'            : 1,
        'init'            : 'random'
    }

    PREC_ESTIM_OPTIONS = ('sample', 'olse')

    RESERVED_STAN_PARAMETER_NAMES = ['X', 'y', 'N', 'D', 'mu_phi', 'Omega_phi']

    def __init__(self, index, stan_model, dphi, X, y, A=None, _master=None, **options):
        opt, sampler = _sort_keywords(options, (self.DEFAULT_OPTIONS, self.DEFAULT_STAN_PARAMS),
                                      "Unexpected option '{}'")
        # sampler settings first: `init_prev` constrains `init`
        self.stan_params = sampler
        self.init_prev = opt['init_prev']
        if self.init_prev:
            self.init_orig = sampler['init']
            if not isinstance(self.init_orig, str):
                raise ValueError("Arg. `init` has to be a string if "
                                 "`init_prev` is True")
        self.prec_estim = opt['prec_estim']
        if self.prec_estim not in self.PREC_ESTIM_OPTIONS:
            raise ValueError("Invalid value for option `prec_estim`")
        self.prec_estim_skip = opt['prec_estim_skip'] if self.prec_estim != 'sample' else 0
        self.verbose = opt['verbose']

        self.index = index
        self.stan_model = stan_model
        self.dphi = dphi
        self.data = dict(N=X.shape[0], X=X, y=y, **(A or {}))
        if X.ndim == 2:
            self.data['D'] = X.shape[1]
        self.phase = 0
        self.iteration = 0
        self.nsamp = None
        self.Q = self.r = None
        self.last_time = self.last_msteps = self.last_mrhat = None
        self.saved_samples = None
        self._Mat = np.zeros((dphi, dphi), order='F')
        self._vec = np.zeros(dphi)
        self._stale = False
        # binding to the device engine (a stand-alone Worker owns a 1-site engine)
        self._master = _master
        self._eng = None
        self._k = None           # local site index inside the engine
        self._has_sampled = False
        if _master is None:
            name = _model_name(stan_model)
            self._eng = _engine.HipEngine(name, np.ascontiguousarray(X), y,
                                          np.array([0, X.shape[0]], dtype=np.int64))
            self._k = 0
            if self._eng.d != dphi:
                raise ValueError('dphi = {} does not match model {} (dphi {})'
                                 .format(dphi, name, self._eng.d))

    # ---- lazily mirrored device state
    def _refresh(self):
        if self._stale and self._eng is not None:
            if self.phase == 1:
                M, v = self._eng.get_cavity(self._k)
            elif self.phase == 2:
                M, v, _ = self._eng.get_tilted(self._k)
            else:
                M = v = None
            if M is not None:
                self._Mat[...] = M
                self._vec[...] = v
        self._stale = False

    @property
    def Mat(self):
        self._refresh()
        return self._Mat

    @property
    def vec(self):
        self._refresh()
        return self._vec

    def _sampler_opts(self):
        sp = self.stan_params
        init = sp['init']
        if not isinstance(init, str) and init != 0:
            init = 'prev'          # list of last draws in the reference (method.py:404-406)
        m = self._master
        return _engine.HipEngine.sampler_opts(
            chains=sp['chains'], iter=sp['iter'], warmup=sp['warmup'], thin=sp['thin'],
            init=init, max_depth=m.max_treedepth if m is not None else 10,
            layout=m.layout if m is not None else 0, adapt=m.adapt if m is not None else 'fresh')

    def _cur_estim(self):
        if self.prec_estim == 'sample' or self.prec_estim_skip > 0:
            return 'sample'
        return self.prec_estim

    def cavity(self, Q, r, Qi, ri):
        """Form the cavity distribution (method.py:267-302).

        Returns True if the cavity precision Q - Qi is positive definite."""
        if self._eng is None:
            raise RuntimeError('this site belongs to another rank')
        self.Q = Q
        self.r = r
        ok = self._eng.cavity_site(self._k, Q, r, Qi, ri)
        self._stale = True
        self.phase = 1 if ok else 0
        if not ok:
            # the reference leaves Mat = Q - Qi, vec = r - ri behind (:288-289)
            self._Mat[...], self._vec[...] = self._eng.get_cavity(self._k)
            self._stale = False
        return ok

    def _save_named(self, names):
        """`saved_samp = {name: draws}` for the requested parameter names (method.py:387-392)."""
        eng = self._eng
        theta = eng.get_draws(self._k, all_params=True)
        ng = 1 if eng.g_cnt is None else int(eng.g_cnt[self._k])
        mid, gauss, sg = _engine.site_spec(eng.model)
        self.saved_samp = _site_params.named_draws(mid, eng.D, ng, gauss, sg, theta, list(names))

    def tilted(self, dQi, dri, save_samples=None, seed=None):
        """Estimate the tilted distribution and write the site parameter update
        into `dQi`, `dri` (method.py:305-475).  Returns False if the precision
        estimate is not positive definite (then dQi, dri are zero).

        `save_samples`: parameter names of the site model whose draws are kept in
        `self.saved_samp` (chain-major, not permuted)."""
        if self.phase != 1:
            raise RuntimeError('Cavity has to be calculated before tilted.')
        if self._eng is None:
            raise RuntimeError('this site belongs to another rank')
        self.stan_params['seed'] = stan_seed(seed)
        m = self._master
        injector = m._sample_injector if m is not None else None
        if self.Q is not None:
            self._eng.set_global(self.Q, self.r)      # dQi -= Q, dri -= r use the aliased arrays (:457-458)
        if injector is not None:
            m._draws_injected = True          # (mix_pred: injected draws hold phi only)
            self._refresh_for_injection()
            samp = np.asfortranarray(injector(self.data, self.stan_params))
            ok = bool(self._eng.moments_batch(samp[:, :, None], self._cur_estim(),
                                              k0=self._k, count=1)[0])
            self.last_time, self.last_msteps, self.last_mrhat = 0.25, 0.125, 1.0625
            lastsamp = [{}] * self.stan_params['chains']
        else:
            flags, stats, ms = self._eng.tilted_batch(
                np.array([self.stan_params['seed']]), self._sampler_opts(), self._cur_estim(),
                k0=self._k, count=1)
            ok = bool(flags[0])
            if stats[0, 7] > 0:
                ok = self._void_update()
            self.last_time = ms * 1e-3
            self.last_msteps = stats[0, 0]
            self.last_mrhat = stats[0, 1]
            lastsamp = 'prev'
            self._has_sampled = True
            if save_samples:
                self._save_named(save_samples)
        if self.verbose:
            print('\n   sampling runtime: {:.4}'.format(self.last_time))
            print('    mean stepsize: {:.4}'.format(self.last_msteps))
            print('    max Rhat: {:.4}'.format(self.last_mrhat))
        if self.init_prev:
            self.stan_params['init'] = lastsamp
        self._finish_tilted(ok)
        dQ, dr = self._eng.get_site(_engine.DQI, self._k)
        dQi[...] = dQ
        dri[...] = dr
        return ok

    def tilted_reuse(self, dQi, dri):
        """`tilted` without sampling: the tilted moments under the current cavity from the draws of the site's last
        sampling call, by Pareto-smoothed importance sampling from the cavity they were sampled against (reweight.py;
        include/epx.h: epx_reweight_batch).  Phase rules and outputs of `tilted`; returns (pos_def, khat, wess) -- whether
        to trust them is the caller's decision (`reweight.reuse_ok`).  The engine must have kept that cavity:
        `set_draw_reuse(True)` before the sampling call (`Master.run(reuse=...)` does it); it raises otherwise."""
        if self.phase != 1:
            raise RuntimeError('Cavity has to be calculated before tilted.')
        if self._eng is None:
            raise RuntimeError('this site belongs to another rank')
        if self.Q is not None:
            self._eng.set_global(self.Q, self.r)
        flags, rec, ms = self._eng.reweight_batch(self._cur_estim(), k0=self._k, count=1)
        ok = bool(flags[0])
        self.last_time = ms * 1e-3
        self._finish_tilted(ok)
        dQ, dr = self._eng.get_site(_engine.DQI, self._k)
        dQi[...] = dQ
        dri[...] = dr
        return ok, float(rec[0, _reweight.RW_KHAT]), float(rec[0, _reweight.RW_WESS])

    def diagnostics(self, rank=False):
        """Per-coordinate diagnostics of the draws of this site's last `tilted` on a stand-alone Worker's own engine:
        the (P, DG_COUNT) record of `diagnostics.diagnostics_host` (columns DG_MEAN, DG_VAR, DG_RHAT, DG_ESS, DG_MCSE,
        DG_ESS_SQ), computed on the device (epx_draw_diagnostics).  rank=True: that record and the (P, RD_COUNT) record
        of `diagnostics.rank_diagnostics_host` (columns RD_RHAT, RD_RHAT_BULK, RD_RHAT_FOLD, RD_ESS_BULK, RD_ESS_TAIL;
        epx_draw_rank_diagnostics)."""
        if self._master is not None:
            raise RuntimeError("This site belongs to a Master: use Master.diagnostics()")
        if not self._has_sampled:
            raise RuntimeError("Can not diagnose draws before `tilted` has sampled some.")
        rec = self._eng.draw_diagnostics(k0=self._k, count=1)[0]
        return (rec, self._eng.draw_rank_diagnostics(k0=self._k, count=1)[0]) if rank else rec

    def _void_update(self):
        """A chain of this site started at a non-finite density (its draws are its initial point):
        the site update is dropped like a failed precision estimate (method.py:462-475)."""
        d = self.dphi
        self._eng.set_site(_engine.DQI, self._k, np.zeros((d, d), order='F'), np.zeros(d))
        return False

    def _refresh_for_injection(self):
        """Expose the device cavity as the Stan data of method.py:221-222."""
        M, v = self._eng.get_cavity(self._k)
        self.data['mu_phi'] = v
        self.data['Omega_phi'] = M.T

    def _finish_tilted(self, ok, nsamp=None):
        """The bookkeeping behind a tilted step (method.py:440-475).  `nsamp`: the draws behind the moments where the
        caller has fetched them for a whole batch (`Master.run`)."""
        self.nsamp = self._eng.get_tilted(self._k)[2] if nsamp is None else nsamp
        if self.prec_estim_skip > 0:
            self.prec_estim_skip -= 1
        if ok:
            self.phase = 2
        else:
            self.phase = 0
            if self.init_prev:
                self.init = self.init_orig        # sic: the reference does not reset stan_params (:468)
        self._stale = True
        self.iteration += 1


# ---------------------------------------------------------------------------------------------
# constructor helpers of Master: every check of method.py:674-814, one concern per function

def _partition(N, site_sizes, site_ind_ord, site_ind):
    """Rows -> sites.  Returns (Nk, k_lim, k_ind, order): rows per site, row limits, site of
    every (sorted) row, and the permutation that sorts the rows by site (None: already sorted).
    Precedence of the three descriptions as in the reference (method.py:696-722)."""
    order = None
    if site_sizes is not None:
        Nk = site_sizes
        k_ind = np.repeat(np.arange(len(Nk), dtype=np.int64), np.asarray(Nk, dtype=np.int64))
    elif site_ind_ord is not None:
        k_ind = site_ind_ord
        Nk = np.bincount(k_ind)
    elif site_ind is not None:
        order = np.argsort(site_ind, kind='mergesort')           # stable: rows keep their order inside a site
        k_ind = site_ind[order]
        Nk = np.bincount(k_ind)
    else:
        raise NotImplementedError("Auto clustering not yet implemented")
    k_lim = np.concatenate(([0], np.cumsum(Nk)))
    if k_lim[-1] != N:
        raise ValueError("Site definition does not match with `X`")
    empty = np.nonzero(np.asarray(Nk) == 0)[0]
    if empty.size:
        raise ValueError("Empty sites: {}. Index the sites from 1 to K-1".format(empty))
    if len(Nk) < 2:
        raise ValueError("Distributed EP should be run with at least "
                         "two sites.")
    return Nk, k_lim, k_ind, order


def _additional_data(A, A_n, A_k, N, K):
    """The three dictionaries of extra Stan data (shared, per row, per site; method.py:736-769):
    lengths must fit and no name may be used twice or shadow the built-in data names."""
    taken = list(Worker.RESERVED_STAN_PARAMETER_NAMES)

    def claim(name):
        if name in taken:
            raise ValueError("Additional data name {} clashes.".format(name))
        taken.append(name)

    for name in A:
        claim(name)
    rows = {}
    for name, val in A_n.items():
        if val.shape[0] != N:
            raise ValueError("The shapes of `A_n[{}]` and `X` does not "
                             "match".format(repr(name)))
        claim(name)
        rows[name] = val if val.flags['CARRAY'] else np.ascontiguousarray(val)
    for name, val in A_k.items():
        if len(val) != K:
            raise ValueError("Array-like length mismatch in `A_k` "
                             "(should be: {}, found: {})"
                             .format(K, len(val)))
        claim(name)
    return A, rows, A_k


def _prior_natural(prior, dphi, device):
    """(Q0, r0, dphi) from the `prior` argument: natural parameters, moment parameters or
    None = unit Gaussian of the given size (method.py:772-797)."""
    if prior is None:
        if dphi is None:
            raise ValueError("If arg. `prior` is not provided, "
                             "arg. `dphi` has to be given")
        return np.asfortranarray(np.eye(dphi)), np.zeros(dphi), dphi
    if not isinstance(prior, dict):
        raise TypeError("Argument `prior` is of wrong type")
    if 'Q' in prior and 'r' in prior:
        Q0 = np.asfortranarray(prior['Q'], dtype=np.float64)
        r0 = np.asarray(prior['r'], dtype=np.float64)
    elif 'S' in prior and 'm' in prior:
        try:
            Q0, r0 = invert_normal_params(np.asarray(prior['S'], dtype=np.float64),
                                          np.asarray(prior['m'], dtype=np.float64), device=device)
        except LinAlgError as ex:
            raise ValueError("Argument `prior` is not appropriate") from ex
    else:
        raise ValueError("Argument `prior` is not appropriate")
    if dphi is None:
        dphi = Q0.shape[0]
    if Q0.shape[0] != dphi or r0.shape[0] != dphi:
        raise ValueError("Arg. `dphi` does not match with `prior`")
    return Q0, r0, dphi


def _damping_schedule(df0, K):
    """Initial damping factor of iteration i as a function (method.py:800-814)."""
    if df0 is None:
        return lambda i, _v=1 / K: _v
    if isinstance(df0, (float, int)):
        if not 0 < df0 <= 1:
            raise ValueError("Constant initial damping factor has to be "
                             "in (0,1]")
        return lambda i, _v=df0: _v
    return df0


# ---------------------------------------------------------------------------------------------
# what the stages of Master.run hand each other

# A tilted step over a rank's sites: per site whether the update stands, the time (s), mean step size and largest R-hat
# reported for it; `reuse_entry`: the step's entry of `Master.reuse_log` (None: draw reuse is off).
_Tilted = namedtuple('_Tilted', 'posdefs times msteps mrhats reuse_entry')


class _Reuse(object):
    """Draw reuse inside ONE `Master.run` call: the policy (keywords of `reweight.reuse_ok`), whether the call's last
    sampling launch left usable draws and their cavities on the device, and the step sizes and R-hats of that launch,
    which a reused iteration reports again."""

    def __init__(self, policy):
        self.policy = policy
        self.have_draws = False
        self.msteps = self.mrhats = None

    def keep(self, msteps, mrhats, usable):
        self.msteps, self.mrhats, self.have_draws = msteps, mrhats, usable


class Master(object):
    """Manages the distributed EP algorithm (method.py:478-1247).

    Parameters are those of the reference (site_model, X, y, A, A_n, A_k,
    site_ind, site_ind_ord, site_sizes, dphi, prior, init_site, df0, df_decay,
    df_treshold, overwrite_model, plus the worker options chains, iter, warmup,
    thin, init, init_prev, prec_estim, prec_estim_skip, verbose).  `site_model`
    is a path or name whose basename selects a built-in GPU site model
    (`m1b_sg` ... `m5b_sg`).

    GPU-only keyword arguments: `device` (HIP device index, default: rank's
    LOCAL_RANK or 0), `comm` (a `dist.EpxComm` to shard the sites over several
    GPUs), `max_treedepth` (default 10), `layout` (0 auto, 1 block per site,
    2 block per (site, chain), 3 streaming), `sync_sites` (gather the site arrays
    of all ranks into the host mirrors when `run` returns, default True),
    `balance_sites` (dispatch the sites of an iteration in decreasing order of the
    leapfrogs they took in the previous one; results do not depend on it, default True),
    `adapt`: 'fresh' (default; every site update adapts step size and metric from scratch like
    the reference's fresh `model.sampling` call, util.py:716) or 'carry' (NOT the reference's
    behaviour: a site update starts from the step sizes its chains ended the previous one with
    and from the site's pooled sample variances as metric, warm-up tunes the step size only --
    same target distribution, far fewer leapfrogs; SURVEY.md Appendix A sanctions it as a
    reported opt-in).
    """

    INFO_OK = 0
    INFO_INVALID_PRIOR = 1
    INFO_DF_TRESHOLD_REACHED_GLOBAL = 2
    INFO_DF_TRESHOLD_REACHED_CAVITY = 3
    INFO_ALL_SITES_FAIL = 4

    MIN_EIG_TRESHOLD = 1e-5
    MIN_EIG = 0.5

    DEFAULT_KWARGS = dict(
        A                 = {},
        A_n               = {},
        A_k               = {},
        site_ind          = None,
        site_ind_ord      = None,
        site_sizes        = None,
        dphi              = None,
        prior             = None,
        init_site         = None,
        df0               = None,
        df_decay          = 0.8,
        df_treshold       = 1e-6,
        overwrite_model   = False
    )

    GPU_KWARGS = dict(
        device            = None,
        comm              = None,
        max_treedepth     = 10,
        layout            = 0,
        sync_sites        = True,
        balance_sites     = True,
        adapt             = 'fresh',
        _engine_factory   = None,
    )

    def __init__(self, site_model, X, y, **kwargs):
        own, gpu, w_opt, w_stan = _sort_keywords(
            kwargs, (self.DEFAULT_KWARGS, self.GPU_KWARGS, Worker.DEFAULT_OPTIONS, Worker.DEFAULT_STAN_PARAMS),
            "Unexpected keyword argument '{}'")
        self.worker_options = dict(w_opt, **w_stan)
        self.site_model = site_model
        self.model_name = _model_name(site_model)
        self.max_treedepth = gpu['max_treedepth']
        self.layout = gpu['layout']
        self.sync_sites = gpu['sync_sites']
        self.balance_sites = gpu['balance_sites']
        if gpu['adapt'] not in ('fresh', 'carry'):
            raise ValueError("adapt must be 'fresh' or 'carry'")
        self.adapt = gpu['adapt']
        self.comm = gpu['comm'] if gpu['comm'] is not None else _dist.LocalComm()
        self._sample_injector = None        # test hook: f(data, stan_params) -> (S, d) draws
        self._draws_injected = False        # the last iteration's draws came from the injector (phi only)
        self.last_site_stats = None         # sampler statistics of the last iteration (local sites)
        self.sampling_ms = []               # device time of every sampling launch (this rank)
        self.ngrad_log = []                 # gradient evaluations of every sampling launch (this rank)
        self.pass_log = []                  # passes over the site rows of every sampling launch (per site)
        self.team_pass_log = []             # layout 7: passes the row team made per launch (all sites), else None
        self.sweep_log = []                 # results of `run(..., sweep=...)`, one dict per iteration
        self.reuse_log = []                 # `run(..., reuse=...)`: one dict per iteration of the last such run (this rank)
        self.df_log = []                    # damping factor accepted in every iteration
        self.othertime_log = []             # host time of every update phase (this rank)
        device = gpu['device']
        if device is None:
            device = int(os.environ.get('LOCAL_RANK', '0')) if self.comm.world > 1 else 0

        # ---- the data and its partition into sites
        if X.ndim not in (1, 2):
            raise ValueError("Argument `X` should be one or two dimensional")
        if y.ndim != 1:
            raise ValueError("Argument `y` should be one dimensional")
        if y.shape[0] != X.shape[0]:
            raise ValueError("The shapes of `y` and `X` does not match")
        self.N = X.shape[0]
        self.D = X.shape[1] if X.ndim == 2 else None
        self.Nk, self.k_lim, self.k_ind, order = _partition(
            self.N, own['site_sizes'], own['site_ind_ord'], own['site_ind'])
        self.K = len(self.Nk)
        # sorted, C-contiguous copies for the device; the Workers below still receive slices of the
        # caller's arrays, as in the reference (method.py:829-830)
        self.X = np.ascontiguousarray(X if order is None else X[order])
        self.y = np.ascontiguousarray(y if order is None else y[order])
        self.A, self.A_n, self.A_k = _additional_data(own['A'], own['A_n'], own['A_k'], self.N, self.K)
        self.Q0, self.r0, self.dphi = _prior_natural(own['prior'], own['dphi'], device)
        self.df_decay = own['df_decay']
        self.df_treshold = own['df_treshold']
        self.df0 = _damping_schedule(own['df0'], self.K)

        # ---- this rank's contiguous block of sites + its device engine
        self.k_lo, self.k_hi = _dist.site_range(self.K, self.comm.rank, self.comm.world)
        self.K_local = self.k_hi - self.k_lo
        if self.K_local < 1:
            raise ValueError("more ranks ({}) than sites ({})".format(self.comm.world, self.K))
        r0w, r1w = int(self.k_lim[self.k_lo]), int(self.k_lim[self.k_hi])
        k_lim_local = np.asarray(self.k_lim[self.k_lo:self.k_hi + 1], dtype=np.int64) - r0w
        groups = {}
        self._site_ng = np.ones(self.K, dtype=np.int64)        # groups per site (all sites: mix_pred's record shapes)
        if not self.model_name.endswith('_sg'):
            # several groups per site (K < J, fit.py:310-324): the multi-group programs take the
            # number of groups `J` per site (A_k) and the 1-based group index `j_ind` per row (A_n)
            g_cnt, g_lim = self._site_groups()
            self._site_ng = np.asarray(g_cnt, dtype=np.int64)
            glo = int(np.sum(g_cnt[:self.k_lo]))
            ghi = glo + int(np.sum(g_cnt[self.k_lo:self.k_hi]))
            groups = dict(g_cnt=g_cnt[self.k_lo:self.k_hi], g_lim=g_lim[glo:ghi + 1] - r0w)
        factory = gpu['_engine_factory']
        if factory is None:
            self.engine = _engine.HipEngine(self.model_name, self.X[r0w:r1w], self.y[r0w:r1w],
                                            k_lim_local, device=device, **groups)
        else:
            self.engine = factory(self.model_name, self.X[r0w:r1w], self.y[r0w:r1w], k_lim_local, **groups)
        if self.engine.d != self.dphi:
            raise ValueError("Arg. `dphi`/`prior` ({}) does not match site model {} (dphi {})"
                             .format(self.dphi, self.model_name, self.engine.d))
        # the draw queries: the engine's own methods, the host route for those it does not have
        self._queries = _dq.Queries(_dq.HostDraws(
            lambda: self.engine, self._site_spec(), self.D, self._site_ng[self.k_lo:self.k_hi], self.X[r0w:r1w], self.y[r0w:r1w],
            np.asarray(self.A_n['j_ind'])[r0w:r1w] if groups else None, k_lim_local, w_stan['chains']))
        if hasattr(self.comm, 'bind'):
            self.comm.bind(self.engine)                   # RCCL communicator of the engine's context (collective)
        # the fused update (epx_update_trial) needs the engine's own communicator (or one rank)
        self._fused = bool(getattr(self.comm, 'native', False)) and hasattr(self.engine, 'update_trial')
        self._host_sums = None

        # ---- workers (method.py:817-834); slices of the ORIGINAL X, y like the reference
        self.workers = []
        for k in range(self.K):
            rows = slice(self.k_lim[k], self.k_lim[k + 1])
            A = dict((key, val[rows]) for (key, val) in self.A_n.items())
            A.update(self.A)
            A.update((key, val[k]) for (key, val) in self.A_k.items())
            w = Worker(k, self.site_model, self.dphi, X[rows], y[rows], A=A, _master=self, **self.worker_options)
            if self.k_lo <= k < self.k_hi:
                w._eng = self.engine
                w._k = k - self.k_lo
            self.workers.append(w)

        # ---- host mirrors (method.py:838-851)
        d, K = self.dphi, self.K
        self.S = np.empty((d, d), order='F')
        self.m = np.empty(d)
        self.Q = self.Q0.copy(order='F')
        self.r = self.r0.copy()
        self.Qi, self.Qi2, self.dQi = (np.zeros((d, d, K), order='F') for _ in range(3))
        self.ri, self.ri2, self.dri = (np.zeros((d, K), order='F') for _ in range(3))
        init_site = own['init_site']
        if isinstance(init_site, np.ndarray):
            self.Qi[...] = init_site[:, :, None]
        elif init_site is not None:
            self.Qi[np.arange(d), np.arange(d), :] = K / (init_site**2)
        self.iter = 0

        # ---- initial global approximation and cavities on the device (method.py:867-882)
        self.engine.set_prior(self.Q0, self.r0)
        self._upload_sites()
        g_pd, c_pd = self._trial(0.0, True)[:2]
        if not g_pd:
            raise ValueError("Initial approximation is not pos.def.")
        if not c_pd:
            raise ValueError("Initial cavity is not pos.def.")
        self.Q[...], self.r[...] = self.engine.get_global()
        for w in self.workers[self.k_lo:self.k_hi]:
            w.Q, w.r = self.Q, self.r
            w.phase = 1
            w._stale = True

    # ------------------------------------------------------------------
    def _trial(self, df, reduce_sums, stat_sum=(), stat_max=(), want_moments=False):
        """One damping trial over all ranks: (global_pd, cav_pd, first_bad (global site or -1),
        stat_sum, stat_max, S, m).  The device engine runs it as one stream-ordered batch with the
        all-reduce inside (epx_update_trial); other engines / transports compose it from the
        engine's primitives and the communicator's host collectives."""
        eng, comm = self.engine, self.comm
        if self._fused:
            return eng.update_trial(df, reduce_sums, self.k_lo, stat_sum, stat_max, want_moments)
        ss = np.array(stat_sum, dtype=np.float64)
        sm = np.array(stat_max, dtype=np.float64)
        if reduce_sums:
            self._host_sums = comm.allreduce_sum(np.array(eng.site_sums(), dtype=np.float64))
            if ss.size:
                ss = comm.allreduce_sum(ss)
            if sm.size:
                sm = comm.allreduce_max(sm)
        g_pd, c_pd, first_bad = eng.damped_trial(df, self._host_sums)
        c_pd = bool(g_pd and c_pd)
        first = self.k_lo + first_bad if (g_pd and first_bad >= 0) else self.K + 1
        if comm.world > 1:
            c_pd = bool(comm.allreduce_min_int(1 if c_pd else 0))
            first = comm.allreduce_min_int(first)
        S = m = None
        if want_moments and g_pd and c_pd:
            S, m = eng.global_moments()
        return g_pd, c_pd, (first if first <= self.K else -1), ss, sm, S, m

    def _upload_sites(self):
        lo, hi = self.k_lo, self.k_hi
        self.engine.set_sites(_engine.QI, np.asfortranarray(self.Qi[:, :, lo:hi]),
                              np.asfortranarray(self.ri[:, lo:hi]))
        self.engine.set_sites(_engine.DQI, np.asfortranarray(self.dQi[:, :, lo:hi]),
                              np.asfortranarray(self.dri[:, lo:hi]))

    def _download_sites(self):
        lo, hi = self.k_lo, self.k_hi
        for which, (Qa, ra) in ((_engine.QI, (self.Qi, self.ri)),
                                (_engine.QI2, (self.Qi2, self.ri2)),
                                (_engine.DQI, (self.dQi, self.dri))):
            Ql, rl = self.engine.get_sites(which)
            if self.comm.world > 1 and self.sync_sites:
                Qa[...] = self.comm.allgather_sites(Ql, self.K)
                ra[...] = self.comm.allgather_sites(rl, self.K)
            else:
                Qa[:, :, lo:hi] = Ql
                ra[:, lo:hi] = rl
        self.Q[...], self.r[...] = self.engine.get_global()

    def mix_phi(self, out_S=None, out_m=None):
        """Posterior approximation of phi from the pooled tilted samples of the last iteration
        (method.py:1250-1296): mean of the site means and the pooled covariance
        `(sum_k scatter_k + sum_k n_k (m_k - m)(m_k - m)') / (n_tot - 1)`.  The reference walks the
        workers' saved samples; here the per-site tilted means / scatters are already on the
        device, so three sums over the sites (and one all-reduce) give the same numbers."""
        if self.iter == 0:
            raise RuntimeError("Can not mix samples before at least one iteration has been done.")
        d, K = self.dphi, self.K
        sums = self.comm.allreduce_sum(self.engine.mix_sums())
        n = self.engine.get_tilted(0)[2]                # draws per site (the same for every site)
        sS = sums[:d * d].reshape(d, d, order='F')
        sm = sums[d * d:d * d + d]
        smm = sums[d * d + d:].reshape(d, d, order='F')
        m = sm / K
        S = (sS + n * (smm - K * np.outer(m, m))) / (n * K - 1)
        if out_S is None:
            out_S = np.zeros((d, d), order='F')
        if out_m is None:
            out_m = np.zeros(d)
        out_S[...] = S
        out_m[...] = m
        return out_S, out_m

    def _need_draws(self, what, refusal):
        """Refuses what reads the draws of the last iteration on the device while there are none: `what` can not be done
        before an iteration; injected draws hold phi only, `refusal`."""
        if self.iter == 0:
            raise RuntimeError("Can not {} before at least one iteration has been done.".format(what))
        if self._draws_injected:
            raise RuntimeError("The draws of the last iteration were injected (`_sample_injector`): they hold phi "
                               "only, {}.".format(refusal))

    def _site_spec(self):
        """(b-model id, Gaussian family, single-group program) of the site model, as site_params takes them."""
        return _engine.site_spec(self.model_name)

    def mix_pred(self, params, smap=None, param_shapes=None):
        """Mean and variance of named parameters of the site model from the tilted draws of the last iteration
        (method.py:1304-1478; experiment/fit.py:408-421 calls it for the models' `alpha`, `beta`).

        params: a name or a list of names; smap: per parameter None (every site holds the whole parameter) or, per
        site, the NumPy index of the site's elements in the global parameter (fit._create_pmaps); param_shapes: the
        global shapes, needed with smap.  Returns (mean, var), lists when `params` is a list.

        The reference extracts every draw of every worker's kept `fit`; here the draws are still in device memory,
        the kernel k_named_moments reduces them to per-site (mean, centred sum of squares) records, and only those
        are combined on the host (mix_pred.combine_moments) -- no `save_last_param` needed.  With several ranks the
        records are gathered over the communicator; every rank returns the same result."""
        self._need_draws("mix samples", "named parameters can not be mixed")
        only_one_param = isinstance(params, str)
        if only_one_param:
            params, smap, param_shapes = [params], [smap], [param_shapes]
        params = list(params)
        ns, ms, vs = _dq.gather_named_moments(self.comm, params, (self._site_spec(), self.D, self._site_ng),
                                              *self._queries.named_moments(params))
        mean, var = _dq.mix_moments(ns, ms, vs, params, smap, param_shapes)
        if only_one_param:
            return mean[0], var[0]
        return mean, var

    def mix_quantiles(self, params, probs=(0.025, 0.25, 0.5, 0.75, 0.975), smap=None, param_shapes=None):
        """Quantiles of named parameters of the site model from the tilted draws of the last iteration: the credible
        intervals beside `mix_pred`'s mean and variance (include/epx.h, "Posterior quantiles", states the order of the
        draws and the type-7 quantile, NumPy's `linear`).  The reference has no counterpart: its user extracts every draw
        and calls np.percentile.

        params, smap, param_shapes: as `mix_pred` takes them; probs: probabilities in [0, 1].  Returns, per parameter, an
        array (len(probs),) + shape; a list of them when `params` is a list.

        smap None (parameters every site holds: phi, mu_a, mu_b, sigma_a, sigma_b, sigma): the quantiles of the POOL of
        all sites' draws, as `mix_phi` and `mix_pred` pool them.  The pool fits no chip and, with several ranks, no single
        device: its order statistics are selected by eight counting passes (k_pooled_count), whose integer counts add
        over the ranks exactly.  smap given: every site's own quantiles (k_site_order_stats sorts a site's draws of an
        element in LDS), placed at the site's index; an index that no site fills and an index that several sites fill are
        ValueErrors -- the quantile of a pool of sites is not a function of the sites' quantiles.

        Only order statistics leave the device; the host interpolates (quantiles.interpolate).  An engine without the
        device methods (the CPU oracle the tests inject) goes through the host functions of quantiles.py.  With several
        ranks every rank returns the same result."""
        self._need_draws("mix samples", "named parameters can not be mixed")
        only_one_param = isinstance(params, str)
        if only_one_param:
            params, smap, param_shapes = [params], [smap], [param_shapes]
        params = list(params)
        maps = [smap[ip] if smap is not None else None for ip in range(len(params))]
        S = int(self.engine.get_tilted(0)[2])               # draws per site (the same for every site)
        sites = (self._site_spec(), self.D, self._site_ng)
        result = [None] * len(params)

        pooled = [par for par, mp in zip(params, maps) if mp is None]
        if pooled:
            ranks, plan = _quantiles.rank_plan(S * self.K, probs)
            stats = _dq.pooled_order_stats(self._queries, self.comm, pooled, _dq.pooled_shapes(*sites, pooled), ranks)
            for ip, par in enumerate(params):
                if maps[ip] is None:
                    result[ip] = _quantiles.interpolate(stats[par], ranks, plan)

        mapped = [par for par, mp in zip(params, maps) if mp is not None]
        if mapped:
            ranks, plan = _quantiles.rank_plan(S, probs)
            if param_shapes is None or any(param_shapes[ip] is None for ip in range(len(params)) if maps[ip] is not None):
                raise ValueError("Arg. `param_shapes` has to be given with `smap`")
            stats = _dq.site_order_stats(self._queries, self.comm, mapped, sites, ranks)
            for ip, par in enumerate(params):
                if maps[ip] is not None:
                    result[ip] = _dq.place_site_quantiles(par, stats, ranks, plan, maps[ip], param_shapes[ip])
        if only_one_param:
            return result[0]
        return result

    def predict(self, X_new, site_sizes=None, site_ind=None, j_ind=None, y_new=None):
        """Posterior predictive of new rows from the tilted draws of the last iteration: what the fitted site models
        predict for rows that were not part of the data (the reference has no counterpart: its user extracts every
        draw and re-applies the models' `transformed parameters`).

        X_new (n, D); the site of every row either as `site_sizes` (K counts, rows ordered by site; a site may have
        none) or as `site_ind` (n site indices, any order) -- exactly one of the two, with the constructor's meaning;
        j_ind: the 1-based group of every row within its site, as in `A_n['j_ind']` (needed by the multi-group models,
        refused by the `_sg` ones); y_new: responses of the new rows, for the log predictive density.

        Returns a dict: `mean` (n) the predictive mean of y (of sigmoid(f) for the Bernoulli-logit models, of f for the
        Gaussian ones), `f_mean` and `f_var` (n) mean and variance over the draws of the linear predictor
        f = alpha + x . beta, `lpd` (n) log mean_s p(y | draw s) or None without `y_new`, `n` the draws per site;
        rows in the caller's order.  The draws stay in device memory, the kernel k_predict reduces them to four
        numbers per row.  With several ranks every rank computes the rows of its own sites and one all-reduce makes
        every rank return the same result."""
        self._need_draws("predict", "nothing can be predicted from them")
        if (site_sizes is None) == (site_ind is None):
            raise ValueError("Give exactly one of `site_sizes` and `site_ind`")
        X_new = _dq.new_rows(X_new, self.D)
        n = X_new.shape[0]
        _, gauss, sg = self._site_spec()
        rows, lim, group = _dq.plan_rows(n, self.K, site_sizes, site_ind, j_ind, self._site_ng, sg, self.model_name)
        ys = _dq.new_responses(y_new, n, gauss, False, self.model_name)
        if ys is not None:
            ys = np.ascontiguousarray(ys[rows])
        Xs = np.ascontiguousarray(X_new[rows])
        lo, hi = int(lim[self.k_lo]), int(lim[self.k_hi])
        local = self._queries.predict(Xs[lo:hi], lim[self.k_lo:self.k_hi + 1] - lo,
                                      None if group is None else group[lo:hi], None if ys is None else ys[lo:hi])
        rec = _dq.sum_predict_rows(self.comm, local, lo, hi, n, ys is not None)
        out = np.empty_like(rec)
        out[rows] = rec
        return _dq.predictive_result(out, ys is not None, self.engine.num_draws())

    def predict_quantiles(self, X_new, probs=(0.025, 0.25, 0.5, 0.75, 0.975), site_sizes=None, site_ind=None, j_ind=None,
                          scale='mean', seed=0):
        """Quantiles over the tilted draws of the last iteration of what the fitted site models predict for new rows:
        the credible band of a row's regression line or fitted probability, and for the Gaussian family the predictive
        interval of its response (include/epx.h, enum epx_pred_order, states the definition; the reference has no
        counterpart: its user extracts every draw, re-applies alpha + x . beta and calls np.percentile).

        X_new, site_sizes, site_ind, j_ind: the rows, as `predict` takes them; probs: probabilities in [0, 1]; scale:
          'linear'    the linear predictor f = alpha + x . beta;
          'mean'      what `predict`'s `mean` averages: sigmoid(f) for the Bernoulli-logit models, f for the Gaussian ones.
                      The sigmoid is monotone, so the host maps the order statistics of f through it and interpolates:
                      the type-7 quantile of sigmoid(f);
          'response'  the replicated response f + sigma z, Gaussian family only (a ValueError otherwise: a 0/1 replicate
                      has no useful quantile); seed: of the replicates' counter-based stream -- a replicate depends on
                      (seed, the caller's row index, draw) only, so the result does not depend on `site_sizes` versus
                      `site_ind` or on the number of ranks.

        Returns a dict: `quantiles` (len(probs), n), the type-7 quantiles (NumPy's `linear`) in the caller's row order,
        NaN for a row with a NaN value; `probs`; `scale`; `n` the draws per site.  The draws stay in device memory: the
        kernel k_predict_order forms every row's values on the matrix pipe, sorts them on chip, and only the order
        statistics the probabilities need leave the device (quantiles.rank_plan, quantiles.interpolate).  With several
        ranks every rank computes the rows of its own sites and one all-reduce makes every rank return the same result."""
        self._need_draws("predict quantiles", "nothing can be predicted from them")
        if (site_sizes is None) == (site_ind is None):
            raise ValueError("Give exactly one of `site_sizes` and `site_ind`")
        if scale not in _predict_quantiles.SCALES:
            raise ValueError("`scale`: one of {} (got {!r})".format(_predict_quantiles.SCALES, scale))
        _, gauss, sg = self._site_spec()
        if scale == 'response' and not gauss:
            raise ValueError("scale='response' replicates the response: site model {!r} is Bernoulli-logit, whose 0/1 "
                             "replicate has no useful quantile".format(self.model_name))
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
            raise ValueError("`seed`: an integer in [0, 2^64)")
        X_new = _dq.new_rows(X_new, self.D)
        n = X_new.shape[0]
        if n >= 2 ** 32:
            raise ValueError("{} rows: the replicates' stream counts rows below 2^32".format(n))
        rows, lim, group = _dq.plan_rows(n, self.K, site_sizes, site_ind, j_ind, self._site_ng, sg, self.model_name)
        S = self.engine.num_draws()
        ranks, plan = _quantiles.rank_plan(S, probs)
        in_order = site_sizes is not None                    # rows by site already: `rows` is 0 .. n - 1, nothing to gather
        Xs = np.ascontiguousarray(X_new if in_order else X_new[rows])
        lo, hi = int(lim[self.k_lo]), int(lim[self.k_hi])
        local = self._queries.predict_order_stats(
            Xs[lo:hi], lim[self.k_lo:self.k_hi + 1] - lo, ranks, None if group is None else group[lo:hi],
            what='yrep' if scale == 'response' else 'f', seed=int(seed),
            row_id=np.ascontiguousarray(rows[lo:hi], dtype=np.int64))
        rec = _dq.sum_order_rows(self.comm, local, lo, hi, n)
        stats = rec
        if not in_order:
            stats = np.empty_like(rec)
            stats[rows] = rec
        q = _predict_quantiles.quantiles_of(stats, ranks, plan, scale == 'mean' and not gauss)
        return dict(quantiles=q, probs=np.atleast_1d(np.asarray(probs, dtype=np.float64)).copy(), scale=scale, n=int(S))

    def predict_new_group(self, X_new, group=None, y_new=None, R=1, seed=0):
        """Posterior predictive of rows of groups that were NOT in the data, from the tilted draws of the last iteration
        (the reference has no counterpart; include/epx.h, epx_predict_new_group, states the definition).  The new
        group's own eta, etb are drawn from the model's prior -- normal(0, 1), double_exponential(0, 1) for m5 -- by a
        counter-based stream, `R` independent replicates per draw, and the pool of ALL sites' phi draws is pushed
        through them: N = K x draws per site x R pool members.

        X_new (n, D); group: an integer label in [0, 2^31) per row (None: one group, label 0) -- rows with the same
        label share the latents, and a label names its stream: the same (seed, label) gives the same latents whatever
        else is in the call; y_new: responses of the new rows, for the log predictive densities; seed: of the stream.

        Returns a dict: `mean`, `f_mean`, `f_var`, `lpd` (n) as `predict` returns them, over the N pool members (lpd is
        None without `y_new`); `groups` the sorted distinct labels and `group_lpd` the joint log predictive density of
        each one's responses, log mean_n exp(sum_i ll_ni) over its rows (None without `y_new`) -- the rows of a group
        share the member's latents, so this is NOT the sum of their `lpd`; `n` = N.  Rows in the caller's order.  With
        several ranks every rank runs all rows against its own sites' draws, and one collective of a rank-slotted
        record followed by newgroup.merge in rank order makes every rank return the same result."""
        self._need_draws("predict a new group", "nothing can be predicted from them")
        X_new = _dq.new_rows(X_new, self.D)
        n = X_new.shape[0]
        if group is None:
            group = np.zeros(n, dtype=np.int64)
        group = np.asarray(group)
        if group.shape != (n,) or not np.issubdtype(group.dtype, np.integer):
            raise ValueError("`group`: one integer label per row of `X_new`")
        bad = np.nonzero((group < 0) | (group >= 2 ** 31))[0]
        if bad.size:
            raise ValueError("`group` of row {}: label {} outside [0, 2^31)".format(int(bad[0]), int(group[bad[0]])))
        if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= R <= _newgroup.R_MAX:
            raise ValueError("`R`: an integer number of replicates in 1..{}".format(_newgroup.R_MAX))
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
            raise ValueError("`seed`: an integer in [0, 2^64)")
        ys = _dq.new_responses(y_new, n, self._site_spec()[1], True, self.model_name)
        S = self.engine.num_draws()
        if self.K * S > 2 ** 32:
            raise ValueError("{} sites x {} draws: more than 2^32 pooled draws".format(self.K, S))
        labels, gidx = np.unique(group, return_inverse=True)
        rows, glpd, N = self._queries.predict_new_group(np.ascontiguousarray(X_new), gidx.astype(np.int32), labels, ys,
                                                        seed=int(seed), t0=self.k_lo * S, R=int(R))
        rows, glpd, N = _dq.merge_new_group(self.comm, rows, glpd, N, ys is not None)
        return _dq.predictive_result(rows, ys is not None, N, groups=labels.astype(np.int64),
                                     group_lpd=np.array(glpd) if ys is not None else None)

    def loo(self):
        """Leave-one-out cross-validation of the fitted site models on the rows they were fitted to, from the tilted
        draws of the last iteration: PSIS-LOO with the Pareto k-hat diagnostic, and WAIC (include/epx.h, enum epx_loo,
        states the definition; the reference has no counterpart).  The number that compares `m1b` ... `m5b` (or the
        `a` family) on the same data: `predict(X, ..., y_new=y)` gives the in-sample log predictive density, which
        always flatters the larger model.

        What the number means here: the draws of a site come from its TILTED distribution, the cavity (all other
        sites' approximations and the prior) times the site's own likelihood -- EP's approximation of the posterior of
        that site's parameters.  Row i of site k is held out by importance-weighting the draws of site k with
        1 / p(y_i | draw); the other sites enter through the cavity, which is kept as it is.  The leave-one-out is
        therefore CONDITIONAL on the EP approximation: it is the exact LOO of the model only as far as the tilted
        distributions are the exact posterior marginals, and it does not propagate the removal of a row into the
        shared parameters' cavity.  A k-hat above the threshold says that the importance weights of that row are too
        heavy-tailed for its estimate to be trusted at this number of draws.

        Returns the dict of `loo.summarise`: the totals `elpd_loo`, `p_loo`, `elpd_waic`, `p_waic` with their standard
        errors `se_*`, the pointwise arrays `lpd`, `elpd_loo_i`, `p_loo_i`, `elpd_waic_i`, `p_waic_i`, `khat`, `wess`,
        `ll_mean` (N each, in the order of the Master's rows: by site), the per-site sums `site_*` (K each), `n` the
        draws per site, `khat_threshold`, `n_bad` and `worst`.

        The draws stay in device memory: the kernel k_loo forms every row's log-likelihoods under its site's draws
        on the matrix pipe, keeps them on chip and reduces them to six numbers per row.  With several ranks every
        rank computes the rows of its own sites and one all-reduce makes every rank return the same result."""
        self._need_draws("cross-validate", "nothing can be cross-validated from them")
        loc, S = self._queries.loo(with_n=True)
        rec = _dq.sum_loo_rows(self.comm, loc, int(self.k_lim[self.k_lo]), int(self.k_lim[self.k_hi]), self.N)
        return _loo.summarise(rec, S, self.k_lim)

    def ppc(self, seed=0, level=0.05, draws=False):
        """Posterior predictive checks of the fitted site models on the rows they were fitted to, from the tilted draws of
        the last iteration (include/epx.h, enum epx_ppc, states the definition; the reference has no counterpart): does
        the model fit the data it was given?  The step between "the chains mixed" (`diagnostics`) and "compare models"
        (`loo`).  For every draw of a site the responses of its rows are replicated from the model, and per group -- one
        (site, group within the site); the site itself for an `_sg` model -- two checks are made: T, the sum of the
        replicated responses against the sum of the observed ones, and D, the realised discrepancy of Gelman, Meng and
        Stern: the log-likelihood of the replicated responses against that of the observed ones under the same draw.

        What the numbers mean here: the draws of a site come from its TILTED distribution, EP's approximation of the
        posterior of that site's parameters, so the check is CONDITIONAL on the EP approximation: a small p-value says
        that the data of the group are unusual under the tilted distribution, whether the model or the approximation is
        at fault.  Draw s of one site and draw s of another are not a draw of anything: a statistic that pairs them has
        no meaning, which is why there are records per group and per site and no whole-data total.

        seed: of the replicates' counter-based stream -- a replicate depends on (seed, row, draw) only, so the result
        does not depend on the number of ranks; level: a group is listed in `extreme` when `p_t` or `p_d` lies outside
        [level / 2, 1 - level / 2]; draws: also return the per-draw values.

        Returns the dict of `ppc.summarise`.  Per group, G each, in the order of the Master's groups (by site):
        `group_site`, `t_obs`, `t_rep_mean`, `t_rep_var`, `p_t_ge` = P(T_rep >= T_obs), `p_t` the mid-p
        (P(T_rep >= T_obs) + P(T_rep > T_obs)) / 2, `d_obs_mean`, `d_rep_mean`, `p_d` = P(D_rep <= D_obs); per site, K
        each, the same under `site_*` (a site's per-draw values are the sums of its groups'); `n` the draws per site;
        `level`; `extreme`; with draws=True `draws` (G, 3, n): T_rep, D_obs, D_rep of every (group, draw) -- on one rank
        only: with several ranks it is refused.  A group with a non-finite linear predictor or log-likelihood has NaN
        everywhere and is not listed in `extreme`.

        The draws stay in device memory: the kernel k_ppc replicates and adds up a group's rows per draw on chip and
        reduces them to eight numbers per group.  With several ranks every rank checks its own sites and the records
        are gathered over the communicator: every rank returns the same dict."""
        self._need_draws("check replicated data", "nothing can be replicated from them")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
            raise ValueError("`seed`: an integer in [0, 2^64)")
        if draws and self.comm.world > 1:
            raise ValueError("`draws=True` returns this rank's per-draw values: with {} ranks it is refused (run on one "
                             "rank, or use `get_draws`)".format(self.comm.world))
        if self.N >= 2 ** 32:
            raise ValueError("{} rows: the replicates' stream counts rows below 2^32".format(self.N))
        got = self._queries.replicated_checks(seed=int(seed), row0=int(self.k_lim[self.k_lo]), with_n=True,
                                              with_draws=bool(draws))
        groups, sites, n = got[0], got[1], got[-1]
        groups, sites, ns = _dq.gather_checks(self.comm, self._site_ng, self.k_lo, groups, sites, n)
        return _ppc.summarise(groups, sites, int(ns[0]), self._site_ng, level, got[2] if draws else None)

    def log_evidence(self, seed=0):
        """The EP approximation of the log marginal likelihood log p(y) of the whole model at the CURRENT approximation
        (include/epx.h, epx_site_evidence, states the per-site definition; the reference has no counterpart): what ranks
        the five nested models as whole models, where `loo` scores rows.  EP's evidence is log Z_EP = Phi(Q, r) -
        Phi(Q0, r0) + sum_k [log Z_k + Phi(Q - Qi_k, r - ri_k) - Phi(Q, r)], Phi the log normaliser of a Gaussian in
        natural parameters (`evidence.log_partition`) and Z_k the integral of site k's likelihood and latent prior against
        its normalised cavity.  Z_k has no closed form: it is estimated per site on the device by bridge sampling between
        the site's tilted draws and a Gaussian proposal fitted to them (`evidence.site_evidence_host` states it in NumPy).

        The value belongs to the approximation the Master holds now.  It is the fixed-point value of EP's evidence only
        once EP has converged: at an earlier iteration the sites and the cavities do not yet agree, and the number moves
        with further iterations.

        seed: of the sampling launch's per-site seeds and of the proposal draws' counter-based stream; a proposal draw
        depends on (seed, site, draw, coordinate) only, so the per-site estimates do not depend on the number of ranks
        given the draws.  The seed does NOT make the call reproducible: with the default `init_prev` the launch starts
        every chain from the last positions of the sampling call before it, so two calls in a row with the same seed
        sample different draws and return values that differ by the estimate's Monte-Carlo error (with the oracle engine
        on two small sites: -16.9136, then -16.9058).

        This launches one sampling call of this rank's sites with the workers' own sampler options against the current
        cavities -- no moment stage: `dQi`, `dri`, the tilted moments and `iter` are untouched.  AFTERWARDS THE DRAWS OF
        THE LAST SAMPLING CALL ARE THIS LAUNCH'S, with the same number of draws per site: `mix_pred`, `loo`, `ppc` and the
        other draw queries then read draws against the current cavities, not those of the last iteration.  It also
        changes where the next `run` iteration starts: with `init_prev` its chains start from this launch's last
        positions instead of the last iteration's, so a `run` behind a `log_evidence` does not sample the draws it would
        have sampled without it (under `adapt='carry'` the carried step sizes and metrics are this launch's too).

        Refused at iteration 0, with a sample injector set, when a local worker is not in phase 1 (its cavity is not
        the current one), and -- a ValueError that names the iterations the sampler needs -- when the first half of the
        chains holds fewer than 2 P draws for the proposal's covariance.

        Returns a dict, the same on every rank: `log_evidence`; per site, K each: `site_log_z` (log Z_k against the
        normalised cavity and the normalised latent prior), `re2` (the relative mean-square error of Z_k that treats the
        draws as independent: the chains' autocorrelation is not in it), `khat` (PSIS k-hat of the proposal's importance
        ratios; above 0.7 the proposal's tails are too light for the site), `iters` (bridge iterations, 1001: not
        converged); `n_bad` the sites with a NaN record or 1001 iterations (`log_evidence` is NaN then); `ms` the device
        time of this rank's evidence kernels (the sampling launch in front of them is not in it)."""
        if self.iter == 0:
            raise RuntimeError("Can not estimate the evidence before at least one iteration has been done.")
        if self._sample_injector is not None:
            raise RuntimeError("A sample injector is set (`_sample_injector`): its draws hold phi only, the evidence "
                               "needs draws of every sampled coordinate.")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < MAX_UINT:
            raise ValueError("`seed`: an integer in [0, {})".format(MAX_UINT))
        local_workers = self.workers[self.k_lo:self.k_hi]
        for w in local_workers:
            if w.phase != 1:
                raise RuntimeError("Worker {} is in phase {}: the evidence needs the current cavity of every site "
                                   "(phase 1).".format(w.index, w.phase))
        eng, w0 = self.engine, local_workers[0]
        sp = w0.stan_params
        opts = w0._sampler_opts()
        warmup = sp['iter'] // 2 if sp['warmup'] is None else sp['warmup']
        nkeep = (sp['iter'] - warmup + sp['thin'] - 1) // sp['thin']
        P = int(eng.P)
        if (nkeep // 2) * sp['chains'] < 2 * P:
            need = 2 * -(-2 * P // sp['chains'])
            raise ValueError("the first half of {} chains of {} kept draws holds {} draws, the proposal of P = {} sampled "
                             "coordinates needs {}: sample at least {} kept iterations per chain (iter - warmup >= {} "
                             "at thin = {})".format(sp['chains'], nkeep, (nkeep // 2) * sp['chains'], P, 2 * P, need,
                                                    need * sp['thin'], sp['thin']))
        sseeds = stan_seeds(run_seeds(int(seed), 1, self.K)[0, self.k_lo:self.k_hi])
        eng.sample_batch(sseeds, opts)
        self._draws_injected = False
        rec, ms = _dq.site_evidence_records(self._queries.host, int(seed), int(self.k_lo))
        mid, gauss, _ = self._site_spec()
        local = np.empty((self.K_local, 5))
        for j in range(self.K_local):
            k = self.k_lo + j
            Om = eng.get_cavity(j)[0]
            local[j, 0] = _evidence.site_log_z(rec[j, _evidence.EV_LOGZ], Om,
                                               _evidence.n_latents(mid, self.D, int(self._site_ng[k])), mid)
            local[j, 1:4] = rec[j, [_evidence.EV_RE2, _evidence.EV_KHAT, _evidence.EV_ITERS]]
            local[j, 4] = _evidence.log_partition(self.Q - self.Qi[:, :, k], self.r - self.ri[:, k])
        full = _dq.gather_evidence(self.comm, self.K, local)
        iters = full[:, 3]
        n_bad = int(np.sum(~np.isfinite(full[:, 0]) | (iters > _evidence.MAX_ITERS)))
        return dict(log_evidence=_evidence.combine_parts(self.Q, self.r, self.Q0, self.r0, full[:, 0], full[:, 4]),
                    site_log_z=full[:, 0].copy(), re2=full[:, 1].copy(), khat=full[:, 2].copy(), iters=iters.copy(),
                    n_bad=n_bad, ms=ms)

    def diagnostics(self, rank=False):
        """Per-coordinate diagnostics of the tilted draws of the last iteration (include/epx.h, enum epx_diag, states
        the definition): which site's moments rest on few effective draws, and whether `iter` is large enough.  The
        reference reports one number per site, the largest split-Rhat (`mrhats`); it has no counterpart.

        Returns a dict.  `mean`, `var`, `rhat`, `ess`, `ess_sq`, `mcse`: each (K, Pmax), one row per site over its
        sampled coordinates, the columns `[:dphi]` are phi, NaN behind a site's own coordinates (multi-group sites of
        different sizes) -- the mean and the variance estimate var_plus of a coordinate, its split-Rhat, the effective
        sample size of its mean and of its second moment (x - mean)^2, and the Monte-Carlo standard error of the
        mean.  `n` (K): the used draws per site.  `site_max_rhat` (K): the largest Rhat of a site (NaN entries
        skipped; NaN when all are); `site_min_ess` (K): the smallest of `ess` and `ess_sq`; `worst`: (site,
        coordinate) of the smallest `site_min_ess`, None when there is none.

        The draws stay in device memory, the kernel k_draw_diag reduces them to six numbers per coordinate; an engine
        without `draw_diagnostics` (the CPU oracle the tests inject) hands its draws to `diagnostics.diagnostics_host`.
        With several ranks every rank computes its own sites and the records are gathered over the communicator:
        every rank returns the same result.

        rank=True adds the rank-normalised diagnostics Stan reports since 2019 (include/epx.h, enum epx_rank_diag; kernel
        k_rank_diag, or `diagnostics.rank_diagnostics_host` on an engine without `draw_rank_diagnostics`), gathered the
        same way: `rhat_rank` = max(`rhat_bulk`, `rhat_folded`), `ess_bulk`, `ess_tail`, each (K, Pmax), and
        `site_max_rhat_rank`, `site_min_ess_rank` (K; the smallest of `ess_bulk` and `ess_tail`).  The folded Rhat sees
        chains that agree in location and differ in scale, which `rhat` does not; the tail ESS measures the draws the
        second moments, and so the precision estimate, rest on.  The other entries are those of rank=False."""
        self._need_draws("diagnose draws", "nothing can be diagnosed from them")
        eng = self.engine
        pg = (eng.P - eng.d) // int(self._site_ng[self.k_lo:self.k_hi].max())     # coordinates per group behind phi
        site_P = eng.d + self._site_ng * pg                                       # (K): every site's own coordinates
        out, ns = _dq.gather_diagnostics(self.comm, site_P, *self._queries.draw_diagnostics(with_n=True))
        rank_out = None
        if rank:
            rank_out, _ = _dq.gather_diagnostics(self.comm, site_P, self._queries.draw_rank_diagnostics())
        return _diagnostics.summarise(out, np.rint(ns).astype(np.int64), rank_out)

    # ---- dispatch of the sampling launches: the policy is dispatch.py's, these are its two knobs and what it needs to
    # know of this rank
    LEAD_FRACTION = _dispatch.LEAD_FRACTION
    PIECES_PER_SITE = int(os.environ.get('EPX_PIECES_PER_SITE', '16'))     # (the environment variable: A/B runs only)

    @classmethod
    def _site_schedule(cls, passes, chain_leapfrogs, n_cu=256):
        return _dispatch.site_schedule(passes, chain_leapfrogs, n_cu, cls.LEAD_FRACTION)

    def _one_workgroup_per_cu(self):
        return _dispatch.one_workgroup_per_cu(self.D, int(np.max(np.diff(self.k_lim[self.k_lo:self.k_hi + 1]))))

    def _dispatch_rank(self):
        eng = self.engine
        return _dispatch.Rank(balance=self.balance_sites, has_queue=hasattr(eng, 'set_piece_queue'), K_local=self.K_local,
                              n_cu=eng.cu_count(), one_wg=self._one_workgroup_per_cu(),
                              iter=self.workers[self.k_lo].stan_params['iter'], pieces_per_site=self.PIECES_PER_SITE,
                              lead_fraction=self.LEAD_FRACTION)

    def _apply_dispatch(self, launch=None, piece=None):
        """Hand a `dispatch.Launch`, or the piece queue alone, to the engine: the only place `run` sets them."""
        eng = self.engine
        if launch is not None:
            eng.set_site_order(launch.order)
            eng.set_site_split(launch.n_lead)
            piece = launch.piece
        if piece is not None:
            eng.set_piece_queue(*piece)

    def _site_groups(self):
        """Group structure of the sites from `A_k['J']` and `A_n['j_ind']` (the data the
        reference hands to m*b.stan): groups per site and the row limits of all groups.  The
        rows of a group have to be contiguous and the groups of a site in order -- what
        `util.distribute_groups` produces."""
        if 'J' not in self.A_k or 'j_ind' not in self.A_n:
            raise ValueError("site model {!r} holds several groups per site: give the number of groups per "
                             "site as A_k['J'] and the 1-based group index of every row as A_n['j_ind'] "
                             "(fit.py:310-324), or use the single-group model {!r}"
                             .format(self.model_name, self.model_name + '_sg'))
        g_cnt = np.asarray(self.A_k['J'], dtype=np.int32)
        j_ind = np.asarray(self.A_n['j_ind'])
        lims = [0]
        for k in range(self.K):
            jk = j_ind[self.k_lim[k]:self.k_lim[k + 1]]
            if jk[0] != 1 or jk[-1] != g_cnt[k] or np.any(np.diff(jk) < 0) or np.any(np.diff(jk) > 1):
                raise ValueError("A_n['j_ind'] of site {}: the rows of a group have to be contiguous and the "
                                 "groups numbered 1..J in order".format(k))
            change = np.nonzero(np.diff(jk))[0] + 1
            lims.extend((self.k_lim[k] + change).tolist())
            lims.append(int(self.k_lim[k + 1]))
        return g_cnt, np.asarray(lims, dtype=np.int64)

    def _score_damps(self, damps, m_target, S_target, samp_target):
        """The sweep itself, on the site sums the device / `_host_sums` hold."""
        eng, comm = self.engine, self.comm
        res = eng.damp_sweep(damps, None if self._fused else self._host_sums, m_target, S_target, samp_target)
        if comm.world > 1:
            res[:, 1] = -comm.allreduce_max(-res[:, 1])
        bad = res[:, 1] == 0.0
        res[bad, 2:] = np.nan
        return dict(damps=np.asarray(damps, dtype=np.float64), global_pd=res[:, 0] > 0, cav_pd=res[:, 1] > 0,
                    mses=res[:, 2], kls=res[:, 3], lls=res[:, 4])

    def damp_sweep(self, damps, m_target, S_target, samp_target=None):
        """Score damping factors for the pending site updates `dQi, dri` against a target
        posterior N(m_target, S_target): the loop `for di, df in enumerate(damps)` of
        experiment/find_damp.py:146-173 as ONE batched device call (the proposal is affine in
        `df`, so the site sums are reduced once).  Returns a dict with `mses`, `lls`, `kls`
        (NaN where the proposal or a cavity is not positive definite, as in the reference) and
        the flags `global_pd`, `cav_pd`.  Site parameters, the global approximation and the
        cavities are those of the accepted state again when it returns."""
        self._trial(0.0, True)                  # reduce the sums of the current (Qi, dQi)
        out = self._score_damps(damps, m_target, S_target, samp_target)
        self._trial(0.0, False)                 # the sweep left the last factor's Q, r and cavities behind
        return out

    def cur_approx(self):
        """Current posterior approximation moments (S, m) (method.py:884-896)."""
        return self.engine.invert_normal_params(self.Q, self.r)

    def _ret(self, info, calc_moments, return_analytics, moments, analytics, as_tuple=False):
        out = [info]
        if calc_moments:
            out.append(moments)
        if return_analytics:
            out.append(analytics)
        if len(out) == 1:
            return out[0]
        return tuple(out) if as_tuple else out

    def run(self, niter, calc_moments=True, save_last_param=None, verbose=True,
            return_analytics=False, seed=None, sweep=None, reuse=None):
        """Run the distributed EP algorithm (method.py:899-1247).

        Returns `info`, optionally followed by `(m_phi_s, cov_phi_s)` and
        `(stimes, msteps, mrhats, othertimes)` exactly like the reference
        (a list on the early-exit paths, a tuple on the normal path).

        `save_last_param`: parameter names whose draws of the LAST iteration every worker keeps
        in `saved_samp` (method.py:1011-1016).

        `sweep` (not in the reference's `run`; it is the body of experiment/find_damp.py): a dict
        `damps, m_target, S_target[, samp_target]`; every iteration scores these damping factors
        before its own damped update and appends the result to `self.sweep_log`.

        `reuse` (not in the reference): True, or a dict with `k_max` and / or `min_ess` (`reweight.reuse_ok`).  From the
        second iteration on every rank first reweights the draws of its last sampling launch to the current cavities
        (`HipEngine.reweight_batch`); if every local site passes `reuse_ok`, the iteration takes its tilted moments from
        the reweighting and launches no sampler, otherwise all local sites sample as without `reuse`.  The decision is
        per rank.  `self.reuse_log` gets one dict per iteration: `reused, n_ok, khat_max` (the largest smoothed k-hat),
        `wess_min_frac` (the smallest WESS / S), `ms` (the reweighting kernel).  In a reused iteration `stimes` is the
        reweighting's time and `msteps`, `mrhats` keep the values of the last sampled one."""
        say = print if verbose else (lambda *a, **k: None)
        if niter < 1:
            say("Nothing to do here as provided arg. `niter` is {}".format(niter))
            return self._ret(self.INFO_OK, calc_moments, return_analytics,
                             (None, None), (None, None, None))

        seeds = run_seeds(seed, niter, self.K)                    # :956-960 (per iteration, drawn up front)
        eng = self.engine
        reuse = self._reuse_state(reuse)
        lo, hi = self.k_lo, self.k_hi
        local_workers = self.workers[lo:hi]

        # host mirrors -> device (the caller may have edited them between runs)
        self._upload_sites()
        eng.set_global(self.Q, self.r)

        m_phi_s = cov_phi_s = None
        if calc_moments:
            m_phi_s = np.zeros((niter, self.dphi))
            cov_phi_s = np.zeros((niter, self.dphi, self.dphi))
        stimes = np.zeros(niter)
        msteps = np.zeros(niter)
        mrhats = np.zeros(niter)
        othertimes = np.zeros(niter)
        moments = (m_phi_s, cov_phi_s)
        analytics = (stimes, msteps, mrhats, othertimes)

        def leave(info, as_tuple=False):
            self._download_sites()
            return self._ret(info, calc_moments, return_analytics, moments, analytics, as_tuple)

        for cur_iter in range(niter):
            self.iter += 1
            say("Iter {} starting. Process tilted distributions".format(self.iter))

            # ---- tilted distributions: ONE batched launch over this rank's sites (:1005-1023)
            for w in local_workers:
                if w.phase != 1:
                    raise RuntimeError('Cavity has to be calculated before tilted.')
            sseeds = stan_seeds(seeds[cur_iter, lo:hi])             # :342-346
            step = self._tilted_step(sseeds, local_workers[0]._cur_estim(), reuse)
            if reuse is not None:
                self.reuse_log.append(step.reuse_entry)
            self._finish_workers(step, sseeds, save_last_param if cur_iter == niter - 1 else None)
            n_ok = int(np.sum(step.posdefs))
            start_othertime = time.time()

            # ---- the one reduction per iteration (:1073-1074, affine in df) and the first damping
            # trial behind it; the site counts and the analytics of :1043-1045 ride on the same buffer
            df = self.df0(self.iter)                                # :1060
            g_pd, c_pd, first_bad, ssum, smax, S, m = self._trial(
                df, True, stat_sum=(n_ok, self.K_local - n_ok),
                stat_max=(np.max(step.times), np.max(step.msteps), np.max(step.mrhats)), want_moments=calc_moments)
            if ssum[1] == 0.0:
                say("\rAll sites ok")
            elif ssum[0] > 0:
                say("\rSome sites failed and are not updated")
            else:
                say("\rEvery site failed")
            if ssum[0] == 0.0:                                      # :1033-1040
                return leave(self.INFO_ALL_SITES_FAIL)
            stimes[cur_iter], msteps[cur_iter], mrhats[cur_iter] = smax[0], smax[1], smax[2]   # :1043-1045
            say("Sampling done, max sampling time {}".format(stimes[cur_iter]))

            if sweep is not None:                                   # find_damp.py:146-173
                self.sweep_log.append(self._score_damps(sweep['damps'], sweep['m_target'], sweep['S_target'],
                                                        sweep.get('samp_target')))
                g_pd, c_pd, first_bad, _, _, S, m = self._trial(df, False, want_moments=calc_moments)

            accepted = self._damped_update(df, (g_pd, c_pd, first_bad, S, m), calc_moments, verbose)
            if not isinstance(accepted, tuple):
                return leave(accepted)
            df, S, m = accepted

            eng.accept(df)                                          # :1145-1158
            self.df_log.append(df)
            for w in local_workers:
                w.Q, w.r = self.Q, self.r
                w.phase = 1
                w._stale = True

            if calc_moments:                                        # :1211-1219
                self.S[...] = S
                self.m[...] = m
                np.copyto(m_phi_s[cur_iter], m)
                np.copyto(cov_phi_s[cur_iter], S.T)
                say("Mean and std of phi[0]: {:.3}, {:.3}".format(
                    m_phi_s[cur_iter, 0], np.sqrt(cov_phi_s[cur_iter, 0, 0])))
            othertimes[cur_iter] = time.time() - start_othertime   # :1230
            self.othertime_log.append(othertimes[cur_iter])
            say("Iter {} done.".format(self.iter))

        say("{} iterations done\nTotal limiting sampling time: {}"
            .format(niter, stimes.sum()))
        return leave(self.INFO_OK, as_tuple=True)

    # ---- the stages of `run`
    def _reuse_state(self, reuse):
        """`run`'s argument `reuse` -> the draw-reuse state of that call (None: off).  The state is the call's own: no
        draws are carried from one `run` to the next."""
        if reuse is None or reuse is False:
            return None
        policy = {} if reuse is True else dict(reuse)
        if set(policy) - {'k_max', 'min_ess'}:
            raise ValueError("`reuse`: True or a dict with 'k_max' and / or 'min_ess'")
        if self._sample_injector is not None:
            raise ValueError('`reuse` needs the draws of the device sampler')
        self.engine.set_draw_reuse(True)
        self.reuse_log = []
        return _Reuse(policy)

    def _tilted_step(self, sseeds, estim, reuse):
        """The tilted moments of this rank's sites, left on the device, from the first source that has them: the
        reweighted draws of the last launch, the injector (test hook) or a sampling launch.  Returns a `_Tilted`."""
        self._draws_injected = self._sample_injector is not None
        entry = None
        if reuse is not None:
            entry = dict(reused=False, n_ok=0, khat_max=float('nan'), wess_min_frac=float('nan'), ms=0.0)
            if reuse.have_draws:
                step = self._tilted_reweighted(estim, reuse)
                if step.reuse_entry['reused']:
                    return step
                entry = step.reuse_entry
        if self._sample_injector is not None:
            return self._tilted_injected(sseeds, estim)
        return self._tilted_sampled(sseeds, estim, reuse)._replace(reuse_entry=entry)

    def _tilted_reweighted(self, estim, reuse):
        """The draws of the last sampling launch reweighted to the current cavities.  `reuse_entry['reused']` says
        whether every local site passed `reweight.reuse_ok`: the moments stand only then."""
        eng = self.engine
        flags, rec, ms = eng.reweight_batch(estim)
        khat, wess, S_draws = rec[:, _reweight.RW_KHAT], rec[:, _reweight.RW_WESS], eng.num_draws()
        site_ok = _reweight.reuse_ok(khat, wess, S_draws, **reuse.policy)
        entry = dict(reused=bool(np.all(site_ok)), n_ok=int(np.sum(site_ok)),
                     khat_max=float(np.max(np.where(np.isposinf(khat), -np.inf, khat))),
                     wess_min_frac=float(np.min(wess)) / S_draws, ms=ms)
        return _Tilted(flags, np.full(self.K_local, ms * 1e-3), reuse.msteps, reuse.mrhats, entry)

    def _tilted_injected(self, sseeds, estim):
        """Test hook: draws come from `self._sample_injector(data, stan_params)`
        (same role as the reference's `_sample_stan`, method.py:43) and go
        through the device moment kernel."""
        eng = self.engine
        samples = None
        for j, w in enumerate(self.workers[self.k_lo:self.k_hi]):
            w.stan_params['seed'] = int(sseeds[j])
            w._refresh_for_injection()
            samp = np.asarray(self._sample_injector(w.data, w.stan_params), dtype=np.float64)
            if samples is None:
                samples = np.empty((samp.shape[0], samp.shape[1], self.K_local), order='F')
            samples[:, :, j] = samp
        posdefs = eng.moments_batch(samples, estim)
        n = self.K_local
        return _Tilted(posdefs, np.full(n, 0.25), np.full(n, 0.125), np.full(n, 1.0625), None)

    def _tilted_sampled(self, sseeds, estim, reuse):
        """One sampling launch over this rank's sites, its logs, and the dispatch of the next one."""
        eng = self.engine
        local_workers = self.workers[self.k_lo:self.k_hi]
        w0 = local_workers[0]
        chains = w0.stan_params['chains']
        rank = self._dispatch_rank()
        self._apply_dispatch(piece=_dispatch.first_launch(rank, launched=bool(self.sampling_ms)))
        posdefs, stats, ms = eng.tilted_batch(sseeds, w0._sampler_opts(), estim)
        voided = np.nonzero(stats[:, 7] > 0)[0]
        for j in voided:
            posdefs[j] = local_workers[j]._void_update()
        self.last_site_stats = stats        # (K_local, 8): see epx_site_stat in include/epx.h
        self.sampling_ms.append(ms)
        self.ngrad_log.append(float(stats[:, 3].sum()))
        self.pass_log.append(eng.row_passes(chains))
        # (layout 7: what the row team really did, yielded passes included -- a measurement aid, bench.py)
        self.team_pass_log.append(float(eng.team_passes().sum()) if eng.last_layout() == 7 else None)
        if _dispatch.schedules(rank):
            self._apply_dispatch(_dispatch.next_launch(rank, eng.last_layout(), self.pass_log[-1],
                                                       eng.get_chain_stats(chains)[:, :, 3]))
        if reuse is not None:
            reuse.keep(stats[:, 0], stats[:, 1], usable=voided.size == 0)   # (a voided site's draws are its initial points)
        return _Tilted(posdefs, np.full(self.K_local, ms * 1e-3), stats[:, 0], stats[:, 1], None)

    def _finish_workers(self, step, sseeds, save_param):
        """What `Worker.tilted` leaves behind on every local worker (method.py:440-475) after a batched tilted step;
        `save_param`: the names whose draws the workers keep (`run`'s last iteration)."""
        nsamp = self.engine.get_tilted(0)[2]
        sampled = self._sample_injector is None
        for j, w in enumerate(self.workers[self.k_lo:self.k_hi]):
            w.stan_params['seed'] = int(sseeds[j])
            w.last_time, w.last_msteps, w.last_mrhat = step.times[j], step.msteps[j], step.mrhats[j]
            if w.init_prev:
                w.stan_params['init'] = 'prev' if sampled else [{}] * w.stan_params['chains']
            w._finish_tilted(step.posdefs[j], nsamp)
            if save_param and sampled:
                w._save_named(save_param)

    def _damped_update(self, df0, first_trial, calc_moments, verbose):
        """From the first trial `(g_pd, c_pd, first_bad, S, m)` at `df0`: decay the damping factor until the global
        approximation and every cavity are positive definite, below `df_treshold` shift the sites once (`force_pd`)
        and start over.  Returns the accepted `(df, S, m)`, or the info code that ends the run."""
        say = print if verbose else (lambda *a, **k: None)
        df = df0
        g_pd, c_pd, first_bad, S, m = first_trial
        say("Iter {}, starting df {:.3g}".format(self.iter, df))
        fail_printline = False
        failed_force_pos_def = False
        while not (g_pd and c_pd):                              # :1067
            df *= self.df_decay                                 # :1083 / :1163
            if verbose:
                fail_printline = True
                if not g_pd:
                    sys.stdout.write("\rNon pos. def. posterior cov, " +
                                     "reducing df to {:.3}".format(df) + " "*5 + "\b"*5)
                else:
                    sys.stdout.write("\rNon pos. def. cavity, " +
                                     "(first encountered in site {}), ".format(first_bad) +
                                     "reducing df to {:.3}".format(df) + " "*5 + "\b"*5)
                sys.stdout.flush()
            if not g_pd and self.iter == 1:                     # :1092-1101
                say("\nInvalid prior.")
                return self.INFO_INVALID_PRIOR
            refresh = False
            if df < self.df_treshold:                           # :1102-1132 / :1177-1207
                say("\nDamping factor reached minimum.")
                df = self.df0(self.iter)
                if failed_force_pos_def:
                    say("Failed to force pos_def.")
                    return self.INFO_DF_TRESHOLD_REACHED_CAVITY
                failed_force_pos_def = True
                forced = self.engine.force_pd(df, self.MIN_EIG_TRESHOLD, self.MIN_EIG)
                say("Force sites {} pos_def.".format(np.nonzero(forced)[0] + self.k_lo))
                refresh = True                                  # the shift changed Qi: reduce the sums again
            g_pd, c_pd, first_bad, _, _, S, m = self._trial(df, refresh, want_moments=calc_moments)
        if fail_printline:
            print()
        return df, S, m
