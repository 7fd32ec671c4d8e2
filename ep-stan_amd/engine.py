"""Device engine: one `epx_ctx` (one rank's sites on one MI355X) behind ctypes.

`HipEngine` is the only engine the package ships.  It raises when libepx.so or
a HIP device is missing -- there is no CPU path.  (Tests drive `Master`'s host
logic on CPU with an oracle-backed engine, oracle/engine_oracle.py, which only tests import.)
"""

import ctypes

import numpy as np

from . import _lib
from . import diagnostics as _diagnostics
from . import evidence as _evidence
from . import loo as _loo
from . import ppc as _ppc
from . import predict_quantiles as _predict_quantiles
from . import site_params as _site_params
from ._lib import SamplerOpts, check, dptr

MODEL_IDS = {'m1b_sg': 0, 'm2b_sg': 1, 'm3b_sg': 2, 'm4b_sg': 3, 'm5b_sg': 4,
             # the multi-group programs experiment/models/m{1..5}b.stan (K < J): same densities with
             # several (eta, etb) blocks per site; they need the group structure of the sites
             'm1b': 0, 'm2b': 1, 'm3b': 2, 'm4b': 3, 'm5b': 4,
             # Gaussian-likelihood family experiment/models/m{1..5}a_sg.stan: phi = [log sigma | the
             # b-model's phi], real responses
             'm1a_sg': 5, 'm2a_sg': 6, 'm3a_sg': 7, 'm4a_sg': 8, 'm5a_sg': 9,
             'm1a': 5, 'm2a': 6, 'm3a': 7, 'm4a': 8, 'm5a': 9}


def is_gauss(model):
    return MODEL_IDS[model] >= 5


def site_spec(model):
    """(b-model id, Gaussian family, single-group program) of a site model, as site_params takes them."""
    return MODEL_IDS[model] % 5, is_gauss(model), model.endswith('_sg')


PREC_ESTIM_IDS = {'sample': 0, 'olse': 1}
QI, QI2, DQI = 0, 1, 2
INIT_IDS = {'random': 0, '0': 1, 0: 1, 'prev': 2}
N_STAT = 8


def model_dims(model, D):
    """(dphi, P) of a single-group logistic model (m*b_sg.stan)."""
    lib = _lib.load()
    d, P = ctypes.c_int(), ctypes.c_int()
    check(lib.epx_model_dims(MODEL_IDS[model], int(D), ctypes.byref(d), ctypes.byref(P)))
    return d.value, P.value


def _f64(a, order='F'):
    return np.require(a, dtype=np.float64, requirements=['F' if order == 'F' else 'C', 'A'])


class HipEngine(object):
    """Sites k = 0..K_local-1 of one rank, resident in HBM."""

    def __init__(self, model, X, y, k_lim, device=0, g_cnt=None, g_lim=None):
        """g_cnt (K) groups per site and g_lim (sum+1) row limits of all groups: sites that hold
        several groups of the hierarchical model (util.distribute_groups, K < J)."""
        self.lib = _lib.load()
        if model not in MODEL_IDS:
            raise ValueError('unknown site model {!r}; built-in models: {}'
                             .format(model, sorted(MODEL_IDS)))
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError('the built-in site models need a two dimensional X')
        gauss = is_gauss(model)
        y32 = None if gauss else np.ascontiguousarray(y, dtype=np.int32)
        yd = np.ascontiguousarray(y, dtype=np.float64) if gauss else None
        k_lim = np.ascontiguousarray(k_lim, dtype=np.int64)
        self.model = model
        self.K = k_lim.shape[0] - 1
        self.D = X.shape[1]
        self.d, self.P = model_dims(model if model.endswith('_sg') else model + '_sg', self.D)
        self.device = device
        self.k_lim = k_lim
        self._trace_sites = 0                  # (set_trace: sites whose transitions are recorded; 0 = off)
        ctx = ctypes.c_void_p()
        if gauss and g_cnt is None:
            if not model.endswith('_sg'):
                raise ValueError('site model {!r} needs the groups of every site (g_cnt, g_lim)'.format(model))
            self.site_P = np.full(self.K, self.P, dtype=np.int64)
            check(self.lib.epx_ctx_create_real(
                device, MODEL_IDS[model], self.K, self.D,
                k_lim.ctypes.data_as(_lib.c_int64_p), dptr(X), dptr(yd), ctypes.byref(ctx)))
        elif g_cnt is None:
            if not model.endswith('_sg'):
                raise ValueError('site model {!r} needs the groups of every site (g_cnt, g_lim)'.format(model))
            check(self.lib.epx_ctx_create(
                device, MODEL_IDS[model], self.K, self.D,
                k_lim.ctypes.data_as(_lib.c_int64_p), dptr(X),
                y32.ctypes.data_as(_lib.c_int32_p), ctypes.byref(ctx)))
        else:
            g_cnt = np.ascontiguousarray(g_cnt, dtype=np.int32)
            g_lim = np.ascontiguousarray(g_lim, dtype=np.int64)
            if g_cnt.shape[0] != self.K or g_lim.shape[0] != int(g_cnt.sum()) + 1:
                raise ValueError('g_cnt needs one entry per site and g_lim sum(g_cnt)+1 entries')
            pg = 1 if MODEL_IDS[model] % 5 == 0 else 1 + self.D
            self.P = self.d + int(g_cnt.max()) * pg          # record stride: the largest site
            self.site_P = self.d + g_cnt.astype(np.int64) * pg
            if gauss:
                check(self.lib.epx_ctx_create_real_groups(
                    device, MODEL_IDS[model], self.K, self.D,
                    k_lim.ctypes.data_as(_lib.c_int64_p), g_cnt.ctypes.data_as(_lib.c_int32_p),
                    g_lim.ctypes.data_as(_lib.c_int64_p), dptr(X), dptr(yd), ctypes.byref(ctx)))
            else:
                check(self.lib.epx_ctx_create_groups(
                    device, MODEL_IDS[model], self.K, self.D,
                    k_lim.ctypes.data_as(_lib.c_int64_p), g_cnt.ctypes.data_as(_lib.c_int32_p),
                    g_lim.ctypes.data_as(_lib.c_int64_p), dptr(X),
                    y32.ctypes.data_as(_lib.c_int32_p), ctypes.byref(ctx)))
        self.g_cnt, self.g_lim = g_cnt, g_lim
        self.ctx = ctx
        n = ctypes.c_int()
        check(self.lib.epx_packed_len(self.ctx, ctypes.byref(n)))
        self.packed_len = n.value

    def close(self):
        if getattr(self, 'ctx', None):
            self.lib.epx_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state transfer
    def set_prior(self, Q0, r0):
        check(self.lib.epx_set_prior(self.ctx, dptr(_f64(Q0)), dptr(_f64(r0))))

    def set_sites(self, which, Q=None, r=None):
        Qa = _f64(Q) if Q is not None else None
        ra = _f64(r) if r is not None else None
        check(self.lib.epx_set_sites(self.ctx, which, dptr(Qa), dptr(ra)))

    def get_sites(self, which, Q=None, r=None):
        """Copy into the given F-ordered arrays (allocated when None)."""
        d, K = self.d, self.K
        if Q is None:
            Q = np.empty((d, d, K), order='F')
        if r is None:
            r = np.empty((d, K), order='F')
        assert Q.flags['F_CONTIGUOUS'] and r.flags['F_CONTIGUOUS']
        check(self.lib.epx_get_sites(self.ctx, which, dptr(Q), dptr(r)))
        return Q, r

    def set_site(self, which, k, Q=None, r=None):
        Qa = _f64(Q) if Q is not None else None
        ra = _f64(r) if r is not None else None
        check(self.lib.epx_set_site(self.ctx, which, int(k), dptr(Qa), dptr(ra)))

    def get_site(self, which, k):
        Q = np.empty((self.d, self.d), order='F')
        r = np.empty(self.d)
        check(self.lib.epx_get_site(self.ctx, which, int(k), dptr(Q), dptr(r)))
        return Q, r

    def set_global(self, Q, r):
        check(self.lib.epx_set_global(self.ctx, dptr(_f64(Q)), dptr(_f64(r))))

    def get_global(self):
        Q = np.empty((self.d, self.d), order='F')
        r = np.empty(self.d)
        check(self.lib.epx_get_global(self.ctx, dptr(Q), dptr(r)))
        return Q, r

    # ---- cavity
    def cavity_batch(self, which, k0=0, count=None):
        count = self.K - k0 if count is None else count
        flags = np.zeros(count, dtype=np.uint8)
        check(self.lib.epx_cavity_batch(self.ctx, which, k0, count,
                                        flags.ctypes.data_as(_lib.c_uint8_p)))
        return flags.astype(bool)

    def cavity_site(self, k, Q, r, Qi, ri):
        flag = ctypes.c_uint8()
        check(self.lib.epx_cavity_site(self.ctx, int(k), dptr(_f64(Q)), dptr(_f64(r)),
                                       dptr(_f64(Qi)), dptr(_f64(ri)), ctypes.byref(flag)))
        return bool(flag.value)

    def get_cavity(self, k):
        Mat = np.empty((self.d, self.d), order='F')
        vec = np.empty(self.d)
        check(self.lib.epx_get_cavity(self.ctx, int(k), dptr(Mat), dptr(vec)))
        return Mat, vec

    # ---- tilted
    @staticmethod
    def sampler_opts(chains=4, iter=1000, warmup=None, thin=1, init='random',
                     max_depth=10, layout=0, flags=0, adapt='fresh'):
        o = SamplerOpts()
        if adapt not in ('fresh', 'carry'):
            raise ValueError("adapt must be 'fresh' (the reference's behaviour) or 'carry'")
        o.reserved = int(flags) | (2 if adapt == 'carry' else 0)    # bit 0: layout 2 without the speculative bookkeeping wave
        o.chains, o.iter, o.thin = int(chains), int(iter), int(thin)
        o.warmup = -1 if warmup is None else int(warmup)
        if init not in INIT_IDS:
            raise ValueError("init must be 'random', '0' or 'prev' for the GPU sampler")
        o.init = INIT_IDS[init]
        o.max_depth, o.layout = int(max_depth), int(layout)
        return o

    def tilted_batch(self, seeds, opts, prec_estim, k0=0, count=None):
        """Returns (posdef bool[count], stats (count, 8), sampling kernel ms)."""
        count = self.K - k0 if count is None else count
        seeds = np.ascontiguousarray(seeds, dtype=np.int64)
        assert seeds.shape[0] == count
        flags = np.zeros(count, dtype=np.uint8)
        stats = np.zeros((count, N_STAT))
        ms = ctypes.c_double()
        check(self.lib.epx_tilted_batch(
            self.ctx, k0, count, seeds.ctypes.data_as(_lib.c_int64_p), ctypes.byref(opts),
            PREC_ESTIM_IDS[prec_estim], flags.ctypes.data_as(_lib.c_uint8_p), dptr(stats),
            ctypes.byref(ms)))
        return flags.astype(bool), stats, ms.value

    def sample_batch(self, seeds, opts, k0=0, count=None):
        count = self.K - k0 if count is None else count
        seeds = np.ascontiguousarray(seeds, dtype=np.int64)
        stats = np.zeros((count, N_STAT))
        ms = ctypes.c_double()
        check(self.lib.epx_sample_batch(self.ctx, k0, count, seeds.ctypes.data_as(_lib.c_int64_p),
                                        ctypes.byref(opts), dptr(stats), ctypes.byref(ms)))
        return stats, ms.value

    # ---- test hook: one teacher-forced transition from checkpoint records (epx_sample_piece)
    CK_SCALARS = ('lps', 'eps', 'da_mu', 's_bar', 'x_bar', 'da_count', 'va_n', 'eps_sum', 'acc_sum', 'depth_sum', 'nleap_tot',
                  'ngrad', 't', 'va_counter', 'va_wsize', 'va_next', 'ndiv', 'npost', 'kept', 'failed')     # csrc/epx_pieces.h EPX_CK_LIST

    def pack_records(self, scalars, qs, wmean, wm2, inv_e):
        """Checkpoint records of the pieced launch from their parts: scalars (..., 20) in CK_SCALARS order and four
        (..., P) vectors -> (..., (4 NV + 1) * 64)."""
        nv = (self.P + 63) // 64
        rec = np.zeros(scalars.shape[:-1] + ((4 * nv + 1) * 64,))
        for j, v in enumerate((qs, wmean, wm2, inv_e)):
            rec[..., j * nv * 64:j * nv * 64 + self.P] = v
        rec[..., 3 * nv * 64 + self.P:4 * nv * 64] = 1.0            # (the metric's padding elements are 1, as the kernels keep them)
        rec[..., 4 * nv * 64:4 * nv * 64 + 20] = scalars
        return rec

    def unpack_records(self, rec):
        nv = (self.P + 63) // 64
        parts = [rec[..., j * nv * 64:j * nv * 64 + self.P] for j in range(4)]
        return rec[..., 4 * nv * 64:4 * nv * 64 + 20], parts[0], parts[1], parts[2], parts[3]

    def sample_piece(self, seeds, opts, t0, records_in):
        """Every chain takes transition t0 of a run with `opts` from the state in records_in (K, chains, record); returns
        the records of boundary t0 + 1."""
        seeds = np.ascontiguousarray(seeds, dtype=np.int64)
        rin = np.ascontiguousarray(records_in, dtype=np.float64)
        out = np.zeros_like(rin)
        check(self.lib.epx_sample_piece(self.ctx, seeds.ctypes.data_as(_lib.c_int64_p), ctypes.byref(opts), int(t0),
                                        dptr(rin), dptr(out)))
        return out

    def moments_batch(self, samples, prec_estim, k0=0, count=None):
        """samples: (S, d, count) F-order -- the injected-draws test hook."""
        count = self.K - k0 if count is None else count
        samples = _f64(samples)
        S = samples.shape[0]
        assert samples.shape[1] == self.d
        flags = np.zeros(count, dtype=np.uint8)
        check(self.lib.epx_moments_batch(self.ctx, k0, count, dptr(samples), S,
                                         PREC_ESTIM_IDS[prec_estim],
                                         flags.ctypes.data_as(_lib.c_uint8_p)))
        return flags.astype(bool)

    # ---- reuse of the draws across iterations (include/epx.h: epx_reweight_batch; reweight.py)
    def set_draw_reuse(self, on):
        """On: every sampling call keeps the cavities it sampled against, for `reweight_batch()` without `theta`."""
        check(self.lib.epx_set_draw_reuse(self.ctx, 1 if on else 0))

    def reweight_batch(self, prec_estim, k0=0, count=None, theta=None, Om_old=None, mu_old=None):
        """The tilted moments and site updates of the sites k0..k0+count under the context's CURRENT cavities from draws
        sampled against older ones, by Pareto-smoothed importance sampling; the results lie where `tilted_batch` leaves
        them.  The draws and their cavities are those of the last sampling call (`set_draw_reuse(True)` before it), or
        `theta` (count, S, P) with `Om_old` (count, d, d) and `mu_old` (count, d).  Returns (posdef bool[count], rec
        (count, 2): columns reweight.RW_KHAT, RW_WESS, kernel ms)."""
        count, theta, S = self._draw_range(k0, count, theta)
        if Om_old is not None:
            Om_old = np.asarray(Om_old, dtype=np.float64)
            if Om_old.shape != (count, self.d, self.d):
                raise ValueError('Om_old: (count, d, d)')
            Om_old = np.ascontiguousarray(Om_old.transpose(0, 2, 1))        # column-major per site
        if mu_old is not None:
            mu_old = np.ascontiguousarray(mu_old, dtype=np.float64)
            if mu_old.shape != (count, self.d):
                raise ValueError('mu_old: (count, d)')
        flags = np.zeros(max(count, 0), dtype=np.uint8)
        rec = np.zeros((max(count, 0), 2))
        ms = ctypes.c_double()
        check(self.lib.epx_reweight_batch(self.ctx, int(k0), int(count), PREC_ESTIM_IDS.get(prec_estim, prec_estim),
                                          dptr(theta), int(S), dptr(Om_old), dptr(mu_old),
                                          flags.ctypes.data_as(_lib.c_uint8_p), dptr(rec), ctypes.byref(ms)))
        return flags.astype(bool), rec, ms.value

    def get_tilted(self, k):
        Mat = np.empty((self.d, self.d), order='F')
        vec = np.empty(self.d)
        n = ctypes.c_int()
        check(self.lib.epx_get_tilted(self.ctx, int(k), dptr(Mat), dptr(vec), ctypes.byref(n)))
        return Mat, vec, n.value

    def num_draws(self):
        n = ctypes.c_int()
        check(self.lib.epx_num_draws(self.ctx, ctypes.byref(n)))
        return n.value

    def get_draws(self, k, all_params=False):
        S = self.num_draws()
        out = np.empty((S, self.P if all_params else self.d), order='F')
        check(self.lib.epx_get_draws(self.ctx, int(k), 1 if all_params else 0, dptr(out)))
        return out

    def get_adapt(self, k, chains):
        """Adaptation history of site k: (final step size per chain, diagonal metric (P))."""
        eps = np.zeros(chains)
        metric = np.zeros(self.P)
        check(self.lib.epx_get_adapt(self.ctx, int(k), dptr(eps), dptr(metric)))
        return eps, metric

    def nuts_transitions(self, seeds, q0, eps, inv_e, nt=1, t_offset=0, layout=0, k0=0):
        """TEST HOOK: nt un-adapted transitions from q0 (count, chains, P)."""
        q0 = np.ascontiguousarray(q0, dtype=np.float64)
        count, chains, P = q0.shape
        assert P == self.P
        seeds = np.ascontiguousarray(seeds, dtype=np.int64)
        eps = np.ascontiguousarray(eps, dtype=np.float64).reshape(count, chains)
        inv_e = np.ascontiguousarray(inv_e, dtype=np.float64).reshape(count, chains, P)
        out = np.zeros((count, chains, nt, P))
        cs = np.zeros((count, chains, N_STAT))
        check(self.lib.epx_nuts_transitions(self.ctx, k0, count, seeds.ctypes.data_as(_lib.c_int64_p),
                                            chains, nt, t_offset, layout, dptr(q0), dptr(eps),
                                            dptr(inv_e), dptr(out), dptr(cs)))
        return out, cs

    def last_layout(self):
        return int(self.lib.epx_last_layout(self.ctx))

    def set_site_order(self, order=None):
        """Scheduling hint: workgroup i of the next full-batch sampling calls takes site order[i]."""
        if order is None:
            check(self.lib.epx_set_site_order(self.ctx, None, 0))
            return
        order = np.ascontiguousarray(order, dtype=np.int32)
        check(self.lib.epx_set_site_order(self.ctx, order.ctypes.data, int(order.shape[0])))

    def set_site_split(self, n_lead):
        """The first `n_lead` sites of the site order run one workgroup per chain, concurrently
        with the others (see include/epx.h: epx_set_site_split)."""
        check(self.lib.epx_set_site_split(self.ctx, int(n_lead)))

    def last_split(self):
        return int(self.lib.epx_last_split(self.ctx))

    def set_piece_queue(self, piece_len=0, rate=None):
        """Piece queue of the resident sampler (include/epx.h: epx_set_piece_queue): the sites' runs in pieces of
        `piece_len` transitions, looping workgroups each claiming the site with the largest remaining predicted work; `rate`: predicted
        leapfrogs per transition of every site (None: all equal); piece_len 0 clears."""
        if rate is not None:
            rate = np.ascontiguousarray(rate, dtype=np.float64)
            if rate.shape != (self.K,):
                raise ValueError('rate: one value per site')
        check(self.lib.epx_set_piece_queue(self.ctx, int(piece_len), None if rate is None else dptr(rate)))

    def set_trace(self, sites=0):
        """Test hook: record every transition (warm-up included) of the first `sites` sites of the next sampling calls."""
        self._trace_sites = int(sites)
        check(self.lib.epx_set_trace(self.ctx, int(sites)))

    def get_trace(self, chains, iter, count=None):
        """(sites, chains, iter, 8 + P): [eps used, leapfrogs, accept, depth, divergent, eps after adaptation,
        sum of the metric, log density, sample] of every transition of the last sampling call's traced sites
        (`count`: the sites that call covered, when it was not all of them)."""
        out = np.zeros((min(self._trace_sites, self.K if count is None else int(count)), int(chains), int(iter), 8 + self.P))
        check(self.lib.epx_get_trace(self.ctx, dptr(out), out.size))
        return out

    def last_segments(self):
        return int(self.lib.epx_last_segments(self.ctx))

    def cu_count(self):
        return int(self.lib.epx_cu_count(self.ctx))

    def row_passes(self, chains, k0=0, count=None):
        """Passes over the site rows made by the last sampling call: in the lock-step layouts (3, 4: streaming / resident
        rows; 7: the row team) the (up to 4) chains of a workgroup share one pass per leapfrog; otherwise every
        gradient is its own pass (over LDS-resident rows)."""
        cs = self.get_chain_stats(chains, k0, count)[:, :, 3]
        if self.last_layout() in (1, 2, 5, 6):
            return cs.sum(axis=1)
        nb = (chains + 3) // 4
        pad = np.zeros((cs.shape[0], nb * 4)); pad[:, :chains] = cs
        return pad.reshape(cs.shape[0], nb, 4).max(axis=2).sum(axis=1)

    def team_passes(self, k0=0, count=None):
        """Layout 7 only: the passes the row team actually made per site, yielded passes included (row_passes() counts the
        gradients of the site's longest chain: a lower bound of this)."""
        count = self.K - k0 if count is None else count
        out = np.zeros(count)
        check(self.lib.epx_get_team_passes(self.ctx, int(k0), int(count), dptr(out)))
        return out

    def get_chain_stats(self, chains, k0=0, count=None):
        count = self.K - k0 if count is None else count
        out = np.zeros((count, chains, N_STAT))
        check(self.lib.epx_get_chain_stats(self.ctx, k0, count, dptr(out)))
        return out

    def logdensity_grad(self, k, theta, layout=2):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        lp = ctypes.c_double()
        g = np.zeros(self.P)
        check(self.lib.epx_logdensity_grad_layout(self.ctx, int(k), dptr(theta), int(layout), ctypes.byref(lp), dptr(g)))
        return lp.value, g

    def invert_normal_params(self, A, b):
        """util.invert_normal_params on this engine's device (new arrays)."""
        from . import util
        return util.invert_normal_params(np.asfortranarray(A, dtype=np.float64),
                                         np.asarray(b, dtype=np.float64), device=self.device)

    # ---- global update
    def site_sums(self):
        """Packed [sum Qi, sum ri, sum dQi, sum dri] of the local sites (NumPy array)."""
        out = np.zeros(self.packed_len)
        check(self.lib.epx_site_sums(self.ctx, dptr(out), None))
        return out

    def damped_trial(self, df, packed=None):
        """One damping trial from host-side packed sums (None: the sums the device holds)."""
        g, c, fb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        if packed is not None:
            packed = np.ascontiguousarray(packed, dtype=np.float64)
        check(self.lib.epx_damped_trial(self.ctx, float(df), dptr(packed), None,
                                        ctypes.byref(g), ctypes.byref(c), ctypes.byref(fb)))
        return bool(g.value), bool(c.value), fb.value

    def update_trial(self, df, reduce_sums, site_base=0, stat_sum=(), stat_max=(), want_moments=False):
        """One damping trial as one stream-ordered batch (epx_update_trial, include/epx.h): site
        sums + all-reduce over the engine's communicator (with `reduce_sums`), global check,
        cavities, flags reduced over the ranks, one synchronisation.  Returns
        (global_pd, cav_pd, first_bad, stat_sum, stat_max, S, m); S, m are None without
        `want_moments`."""
        ss = np.array(stat_sum, dtype=np.float64).reshape(-1)
        sm = np.array(stat_max, dtype=np.float64).reshape(-1)
        g, c, fb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        S = m = None
        if want_moments:
            S = np.empty((self.d, self.d), order='F')
            m = np.empty(self.d)
        check(self.lib.epx_update_trial(
            self.ctx, float(df), 1 if reduce_sums else 0, int(site_base),
            dptr(ss) if ss.size else None, int(ss.size), dptr(sm) if sm.size else None, int(sm.size),
            1 if want_moments else 0, ctypes.byref(g), ctypes.byref(c), ctypes.byref(fb), dptr(S), dptr(m)))
        return bool(g.value), bool(c.value), int(fb.value), ss, sm, S, m

    # ---- the engine's communicator (dist.EpxComm binds it)
    def comm_size(self):
        r, n = ctypes.c_int(), ctypes.c_int()
        check(self.lib.epx_comm_size(self.ctx, ctypes.byref(r), ctypes.byref(n)))
        return r.value, n.value

    def comm_allreduce(self, buf, op):
        assert buf.dtype == np.float64 and buf.flags['C_CONTIGUOUS']
        check(self.lib.epx_comm_allreduce(self.ctx, dptr(buf), int(buf.size), int(op)))
        return buf

    def comm_allgather(self, buf, world):
        buf = np.ascontiguousarray(buf, dtype=np.float64)
        out = np.empty((world, buf.size))
        check(self.lib.epx_comm_allgather(self.ctx, dptr(buf), int(buf.size), dptr(out)))
        return out

    def damp_sweep(self, damps, packed, m_target, S_target, samp_target=None):
        """Score every damping factor of `damps` (find_damp.py:146-173) -> (ndf, 5) array
        [global_pd, cav_pd (this rank's sites), mse, kl, ll]; criteria NaN unless both flags hold.
        packed: the all-reduced site sums (host array), or None for the ones the device holds."""
        damps = np.ascontiguousarray(damps, dtype=np.float64)
        m_t = np.ascontiguousarray(m_target, dtype=np.float64)
        S_t = np.asfortranarray(S_target, dtype=np.float64)
        half_logdet = float(np.sum(np.log(np.diag(np.linalg.cholesky(S_t)))))
        xm = xs = None
        ns = 0
        if samp_target is not None:
            samp = np.asarray(samp_target, dtype=np.float64)
            ns = samp.shape[0]
            xm = np.ascontiguousarray(samp.mean(axis=0))
            c = samp - xm
            xs = np.asfortranarray(c.T.dot(c))
        out = np.zeros((damps.shape[0], 5))
        host = None if packed is None else dptr(np.ascontiguousarray(packed, dtype=np.float64))
        check(self.lib.epx_damp_sweep(self.ctx, int(damps.shape[0]), dptr(damps), host, None, dptr(m_t), dptr(S_t),
                                      half_logdet, dptr(xm) if xm is not None else None,
                                      dptr(xs) if xs is not None else None, int(ns), dptr(out)))
        return out

    def mix_sums(self):
        """[sum_k scatter_k, sum_k mean_k, sum_k mean_k mean_k'] of the local sites' tilted moments."""
        out = np.zeros(2 * self.d * self.d + self.d)
        check(self.lib.epx_mix_sums(self.ctx, dptr(out)))
        return out

    def named_moments(self, names, k0=0, count=None, theta=None):
        """Per-site moments of named parameters of the site model (epx_named_moments, include/epx.h): (n, mean, m2)
        with n the draws per site and mean / m2 lists, one entry per site, of {name: ndarray} -- the mean and the
        centred sum of squares in the per-site shapes of site_params.named_draws.  The draws are those of the last
        sampling call, on the device; `theta` (count, S, P) injects draws instead (test hook)."""
        names, ids = self._named_ids(names)
        count, theta, S = self._draw_range(k0, count, theta)
        lens = self._named_lens(ids, self._widest_site())
        L = int(sum(lens))
        mean = np.zeros((count, L))
        m2 = np.zeros((count, L))
        n = ctypes.c_int()
        check(self.lib.epx_named_moments(self.ctx, int(k0), int(count), ids.ctypes.data_as(_lib.c_int32_p), len(names),
                                         dptr(theta), int(S), dptr(mean), dptr(m2), ctypes.byref(n)))
        return n.value, self._cut_sites(names, lens, mean, k0), self._cut_sites(names, lens, m2, k0)

    def _new_rows(self, Xn, n, group, group_name, y):
        """Xn (n, D) -- n None: any -- as float64, one int32 group per row (or None) and one float64 response per row (or
        None) of predict / predict_new_group."""
        Xn = np.ascontiguousarray(Xn, dtype=np.float64)
        if Xn.ndim != 2 or Xn.shape[1] != self.D or (n is not None and Xn.shape[0] != n):
            raise ValueError('Xn: (n, D) = ({}, {})'.format('n' if n is None else n, self.D))
        if group is not None:
            group = np.ascontiguousarray(group, dtype=np.int32)
            if group.shape != (Xn.shape[0],):
                raise ValueError(group_name + ': one group per new row')
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float64)
            if y.shape != (Xn.shape[0],):
                raise ValueError('y: one response per new row')
        return Xn, group, y

    def predict(self, Xn, row_lim, row_group=None, y=None, k0=0, count=None, theta=None):
        """Posterior predictive of new rows (epx_predict, include/epx.h): (n, 4), columns site_params.PR_MEAN,
        PR_F_MEAN, PR_F_M2, PR_LPD (NaN without y).  Xn (n, D); the rows of site k0 + j are
        [row_lim[j], row_lim[j+1]); row_group (n): 0-based group within the row's site (None: 0).  The draws are those
        of the last sampling call, on the device; `theta` (count, S, P) injects draws instead (test hook)."""
        count = self.K - k0 if count is None else count
        row_lim = np.ascontiguousarray(row_lim, dtype=np.int64)
        if row_lim.shape != (count + 1,):
            raise ValueError('row_lim: count + 1 = {} row limits'.format(count + 1))
        Xn, row_group, y = self._new_rows(Xn, int(row_lim[-1]), row_group, 'row_group', y)
        count, theta, S = self._draw_range(k0, count, theta)
        out = np.zeros((Xn.shape[0], _site_params.PR_COUNT))
        check(self.lib.epx_predict(self.ctx, int(k0), int(count), row_lim.ctypes.data_as(_lib.c_int64_p),
                                   row_group.ctypes.data_as(_lib.c_int32_p) if row_group is not None else None,
                                   dptr(Xn), dptr(y), dptr(theta), int(S), dptr(out), None))
        return out

    def predict_order_stats(self, Xn, row_lim, ranks, row_group=None, what='f', seed=0, row_id=None, k0=0, count=None,
                            theta=None, with_n=False):
        """Order statistics across the draws of new rows (epx_predict_order_stats, include/epx.h): (n, len(ranks)) -- per
        row v_(r) for the 0-based ranks r (ascending, distinct, below the draws per site, at most 32) of v = f (what =
        'f') or of the replicated response f + sigma z (what = 'yrep', Gaussian family only), NaN for a row with a NaN
        value.  Xn, row_lim, row_group: as `predict` takes them; seed: of the replicates' stream; row_id (n): the stream
        index in [0, 2^32) of every row (None: its position in the call).  The draws are those of the last sampling
        call, on the device; `theta` (count, S, P) injects draws instead (test hook).  with_n: also return the draws
        per site."""
        count = self.K - k0 if count is None else count
        row_lim = np.ascontiguousarray(row_lim, dtype=np.int64)
        if row_lim.shape != (count + 1,):
            raise ValueError('row_lim: count + 1 = {} row limits'.format(count + 1))
        Xn, row_group, _ = self._new_rows(Xn, int(row_lim[-1]), row_group, 'row_group', None)
        ranks = np.ascontiguousarray(ranks, dtype=np.int64).ravel()
        if row_id is not None:
            row_id = np.ascontiguousarray(row_id, dtype=np.int64)
            if row_id.shape != (Xn.shape[0],):
                raise ValueError('row_id: one stream index per new row')
        count, theta, S = self._draw_range(k0, count, theta)
        out = np.zeros((Xn.shape[0], ranks.size))
        n = ctypes.c_int()
        check(self.lib.epx_predict_order_stats(
            self.ctx, int(k0), int(count), row_lim.ctypes.data_as(_lib.c_int64_p),
            row_group.ctypes.data_as(_lib.c_int32_p) if row_group is not None else None, dptr(Xn),
            row_id.ctypes.data_as(_lib.c_int64_p) if row_id is not None else None,
            _predict_quantiles.WHAT[what] if what in _predict_quantiles.WHAT else int(what), ctypes.c_uint64(int(seed)),
            ranks.ctypes.data_as(_lib.c_int64_p), int(ranks.size), dptr(theta), int(S), dptr(out), ctypes.byref(n)))
        return (out, n.value) if with_n else out

    def predict_new_group(self, Xn, gidx, labels, y=None, seed=0, t0=0, R=1, k0=0, count=None, theta=None):
        """Posterior predictive of groups that were not in the data (epx_predict_new_group, include/epx.h):
        (rows (n, 4), glpd (G,), N) -- the columns of `predict` over the pool of N = count S R members, and the joint
        log predictive density of every new group's responses (NaN without y).  Xn (n, D); gidx (n): dense index of
        the row's new group (None: 0); labels (G): the stream's label of every group; t0: pooled index of site k0's
        first draw.  The draws are those of the last sampling call, on the device; `theta` (count, S, P) injects
        draws instead (test hook)."""
        Xn, gidx, y = self._new_rows(Xn, None, gidx, 'gidx', y)
        n = Xn.shape[0]
        labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        count, theta, S = self._draw_range(k0, count, theta)
        G = labels.shape[0]
        out = np.zeros((n, _site_params.PR_COUNT))
        glpd = np.zeros(G)
        N = ctypes.c_longlong()
        check(self.lib.epx_predict_new_group(
            self.ctx, int(k0), int(count), ctypes.c_uint64(int(seed)), int(t0), int(R), n, dptr(Xn), dptr(y),
            gidx.ctypes.data_as(_lib.c_int32_p) if gidx is not None else None, G, labels.ctypes.data_as(_lib.c_int32_p),
            dptr(theta), int(S), dptr(out), dptr(glpd), ctypes.byref(N)))
        if n == 0:                                       # nothing launched: groups without rows
            glpd[:] = np.nan if y is None else 0.0
        return out, glpd, N.value

    def newgroup_latents(self, seed, label, t0, nt, R):
        """TEST HOOK: the latents (nt, R, E) of new group `label` at the pooled draws t0..t0+nt (epx_newgroup_latents)."""
        E = 1 if MODEL_IDS[self.model] % 5 == 0 else 1 + self.D
        out = np.zeros((max(int(nt), 0), max(int(R), 0), E))
        check(self.lib.epx_newgroup_latents(int(self.device), MODEL_IDS[self.model], self.D, ctypes.c_uint64(int(seed)),
                                            int(label), int(t0), int(nt), int(R), dptr(out)))
        return out

    def loo(self, k0=0, count=None, theta=None, with_n=False):
        """Leave-one-out records of the context's own rows of the sites k0..k0+count (epx_loo, include/epx.h):
        (rows, 6), columns loo.LO_LPD, LO_LL_MEAN, LO_LL_M2, LO_ELPD, LO_KHAT, LO_WESS, in the context's row order.  The
        draws are those of the last sampling call, on the device; `theta` (count, S, P) injects draws instead (test
        hook).  with_n: also return the draws per site."""
        count, theta, S = self._draw_range(k0, count, theta)
        ok = 0 <= k0 and count >= 1 and k0 + count <= self.K        # (a bad range: the library says so)
        rows = int(self.k_lim[k0 + count] - self.k_lim[k0]) if ok else 0
        out = np.zeros((rows, _loo.LO_COUNT))
        n = ctypes.c_int()
        check(self.lib.epx_loo(self.ctx, int(k0), int(count), dptr(theta), int(S), dptr(out), ctypes.byref(n)))
        return (out, n.value) if with_n else out

    def replicated_checks(self, seed=0, row0=0, k0=0, count=None, theta=None, with_n=False, with_draws=False):
        """Posterior predictive check records of the context's own rows of the sites k0..k0+count (epx_ppc,
        include/epx.h): (groups, sites[, draws][, n]) -- groups (G, 8) one record per (site, group) of the range in the
        context's order and sites (count, 8), columns ppc.PC_T_OBS .. PC_D_LE; with_draws: also the per-draw T_rep, D_obs,
        D_rep of every group, (G, 3, S); with_n: also the draws per site.  seed: of the replicates' stream; row0: the
        stream's row of the context's row 0.  The draws are those of the last sampling call, on the device; `theta`
        (count, S, P) injects draws instead (test hook)."""
        count, theta, S = self._draw_range(k0, count, theta)
        ok = 0 <= k0 and count >= 1 and k0 + count <= self.K        # (a bad range: the library says so)
        G = (int(self.g_cnt[k0:k0 + count].sum()) if self.g_cnt is not None else count) if ok else 0
        Sd = (S if theta is not None else self.num_draws()) if with_draws and ok else 0
        groups, sites = np.zeros((G, _ppc.PC_COUNT)), np.zeros((max(int(count), 0) if ok else 0, _ppc.PC_COUNT))
        draws = np.zeros((G, 3, Sd)) if with_draws else None
        n = ctypes.c_int()
        check(self.lib.epx_ppc(self.ctx, int(k0), int(count), ctypes.c_uint64(int(seed)), int(row0), dptr(theta), int(S),
                               dptr(groups), dptr(sites), dptr(draws), ctypes.byref(n)))
        return (groups, sites) + ((draws,) if with_draws else ()) + ((n.value,) if with_n else ())

    def site_evidence(self, seed=0, site0=0, k0=0, count=None, theta=None, chains=None, with_terms=False):
        """Bridge-sampling records of the sites k0..k0+count (epx_site_evidence, include/epx.h): (out, terms, ms) -- out
        (count, 6), columns evidence.EV_LOGZ, EV_LOGZ_IS, EV_ITERS, EV_RE2, EV_KHAT, EV_N1; terms: None, or with_terms the
        list of every site's dict of `evidence.cut_terms` (l1, l2, m, L, proposal draws; it needs `chains`); ms: the device
        time of the three kernels.  seed: of the proposal draws' stream; site0: the index of the context's first site among all sites.
        The draws are those of the last sampling call, on the device (`chains`, where given, has to be that call's: the
        buffer of the terms is sized by it and the library refuses another value); `theta` (count, S, P), chain-major, with
        `chains` injects draws instead (test hook)."""
        if (theta is not None or with_terms) and chains is None:
            raise ValueError('injected draws, and `with_terms`, need `chains`')
        count, theta, S = self._draw_range(k0, count, theta)
        ok = 0 <= k0 and count >= 1 and k0 + count <= self.K        # (a bad range: the library says so)
        out = np.zeros((max(int(count), 0) if ok else 0, _evidence.EV_COUNT))
        terms = None
        if with_terms and ok:
            Sd, ch = S if theta is not None else self.num_draws(), int(chains)
            N1 = _evidence.split_sizes(Sd, ch)[1] if Sd > 0 and ch > 0 and Sd % ch == 0 else 0
            terms = np.zeros((int(count), _evidence.terms_width(N1, self.P)))
        ms = ctypes.c_double()
        check(self.lib.epx_site_evidence(self.ctx, int(k0), int(count), ctypes.c_uint64(int(seed)), int(site0), dptr(theta),
                                         int(S), 0 if chains is None else int(chains), dptr(out), dptr(terms),
                                         ctypes.byref(ms)))
        if terms is not None:
            terms = [_evidence.cut_terms(row, N1, self.P) for row in terms]
        return out, terms, ms.value

    def psis_rows(self, ll):
        """PSIS of every row of ll (n, S) on this engine's device (epx_psis_rows): (n, 3), columns ELPD, KHAT, WESS."""
        ll = np.ascontiguousarray(ll, dtype=np.float64)
        if ll.ndim != 2 or ll.shape[1] < 1:
            raise ValueError('ll: (n, S) with S >= 1')
        out = np.zeros((ll.shape[0], 3))
        check(self.lib.epx_psis_rows(int(self.device), ll.shape[0], ll.shape[1], dptr(ll), dptr(out)))
        return out

    def draw_diagnostics(self, k0=0, count=None, theta=None, chains=None, with_n=False):
        """Per-coordinate diagnostics of the draws of the sites k0..k0+count (epx_draw_diagnostics, include/epx.h):
        (count, P, 6), columns diagnostics.DG_MEAN, DG_VAR, DG_RHAT, DG_ESS, DG_MCSE, DG_ESS_SQ; NaN behind a
        multi-group site's own `site_P[k]` coordinates.  The draws, chains and nkeep are those of the last sampling
        call, on the device; `theta` (count, S, P), chain-major, with `chains` injects draws instead (test hook).
        with_n: also return the used draws per site."""
        return self._diagnose(self.lib.epx_draw_diagnostics, _diagnostics.DG_COUNT, k0, count, theta, chains, with_n)

    def draw_rank_diagnostics(self, k0=0, count=None, theta=None, chains=None, with_n=False):
        """Rank-normalised diagnostics of the draws of the sites k0..k0+count (epx_draw_rank_diagnostics, include/epx.h):
        (count, P, 5), columns diagnostics.RD_RHAT, RD_RHAT_BULK, RD_RHAT_FOLD, RD_ESS_BULK, RD_ESS_TAIL; NaN behind a
        multi-group site's own `site_P[k]` coordinates.  Draws, `theta`, `chains` and `with_n` as `draw_diagnostics`
        takes them; at most diagnostics.RD_MAX_DRAWS used draws per site."""
        return self._diagnose(self.lib.epx_draw_rank_diagnostics, _diagnostics.RD_COUNT, k0, count, theta, chains, with_n)

    def _diagnose(self, entry, width, k0, count, theta, chains, with_n):
        """The (count, P, width) records of one of the library's two diagnostics entries (and the used draws per site)."""
        if theta is not None and chains is None:
            raise ValueError('injected draws need `chains`')
        count, theta, S = self._draw_range(k0, count, theta)
        out = np.zeros((max(int(count), 0), self.P, width))
        n = ctypes.c_int()
        check(entry(self.ctx, int(k0), int(count), dptr(theta), int(S), int(chains) if theta is not None else 0, dptr(out),
                    ctypes.byref(n)))
        return (out, n.value) if with_n else out

    def rank_normalize(self, x, fold=False):
        """(rank, z) of every row of x (m, n) on this engine's device (epx_rank_normalize, the ranking stage of
        k_rank_diag alone): what diagnostics.rank_normalize_host computes."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] < 1:
            raise ValueError('x: (m, n) with n >= 1')
        rank, z = np.zeros(x.shape), np.zeros(x.shape)
        check(self.lib.epx_rank_normalize(int(self.device), x.shape[0], x.shape[1], dptr(x), 1 if fold else 0,
                                          dptr(rank), dptr(z)))
        return rank, z

    def pooled_moments(self, center=None, k0=0, count=None, theta=None, want_scatter=True):
        """Moments of the phi draws of the sites k0..k0+count pooled (epx_pooled_moments, include/epx.h): (n, sum, scatter)
        with n the number of draws, sum (d) = sum (x - center) and scatter (d, d) = sum (x - center)(x - center)', None
        without `want_scatter`; `center` None = 0.  The draws are those of the last sampling call, on the device;
        `theta` (count, S, P) injects draws instead (test hook)."""
        d = self.d
        count, theta, S = self._draw_range(k0, count, theta)
        if center is not None:
            center = np.ascontiguousarray(center, dtype=np.float64)
            if center.shape != (d,):
                raise ValueError('center: ({},)'.format(d))
        s = np.zeros(d)
        sc = np.zeros((d, d), order='F') if want_scatter else None
        n = ctypes.c_longlong()
        check(self.lib.epx_pooled_moments(self.ctx, int(k0), int(count), dptr(center), dptr(theta), int(S),
                                          1 if want_scatter else 0, dptr(s), dptr(sc), ctypes.byref(n)))
        return n.value, s, sc

    def _named_ids(self, names):
        names = [names] if isinstance(names, str) else list(names)
        for name in names:
            if name not in _site_params.NAME_IDS:
                raise ValueError('unknown parameter name {!r} (known: {})'.format(name, sorted(_site_params.NAME_IDS)))
        return names, np.array([_site_params.NAME_IDS[name] for name in names], dtype=np.int32)

    def _named_lens(self, ids, k):
        """Elements of every name at site k; an undefined name fails in the library like any other error."""
        lens = []
        for i in ids:
            n = ctypes.c_int()
            check(self.lib.epx_named_len(self.ctx, int(k), int(i), ctypes.byref(n)))
            lens.append(n.value)
        return lens

    def _widest_site(self):
        """The site whose lengths size a row of the per-site calls over named parameters."""
        return int(np.argmax(self.g_cnt)) if self.g_cnt is not None else 0

    def _cut_sites(self, names, lens, rows, k0, lead=()):
        """rows (count,) + lead + (L,), every site's names side by side at the widest site's lengths `lens` -> a list, one
        entry per site, of {name: lead + the per-site shape of site_params.named_draws}."""
        mid, gauss, sg = site_spec(self.model)
        off = np.concatenate(([0], np.cumsum(lens)))
        sites, cuts = [], {}                             # cuts: per group count, (name, first, last, shape) of every name
        for b in range(rows.shape[0]):
            ng = 1 if self.g_cnt is None else int(self.g_cnt[k0 + b])
            if ng not in cuts:
                shapes = [_site_params.named_shape(mid, self.D, ng, gauss, sg, name) for name in names]
                cuts[ng] = [(name, o, o + int(np.prod(sh, dtype=np.int64)), lead + sh)
                            for name, o, sh in zip(names, off, shapes)]
            row = rows[b]
            sites.append(dict((name, np.array(row[..., lo:hi], order='C').reshape(shape))      # (np.array: its own copy)
                              for name, lo, hi, shape in cuts[ng]))
        return sites

    def _draw_range(self, k0, count, theta):
        """What every entry over draws opens with: (count, theta, S).  count None: the sites from k0 on; `theta` (count, S,
        P) as the library takes it, and S; (None, 0): the draws of the last sampling call."""
        count = self.K - k0 if count is None else count
        if theta is None:
            return count, None, 0
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.ndim != 3 or theta.shape[0] != count or theta.shape[2] != self.P:
            raise ValueError('theta: (count, S, P) = ({}, S, {})'.format(count, self.P))
        return count, theta, theta.shape[1]

    def named_order_stats(self, names, ranks, k0=0, count=None, theta=None):
        """Per-site order statistics of named parameters of the site model (epx_named_order_stats, include/epx.h): a list,
        one entry per site, of {name: (len(ranks),) + per-site shape} -- x_(r) of every element's draws at that site for
        the 0-based ranks r (ascending, distinct, below the draws per site, at most 32), NaN for an element with a NaN
        draw.  The draws are those of the last sampling call, on the device; `theta` (count, S, P) injects draws instead
        (test hook)."""
        names, ids = self._named_ids(names)
        ranks = np.ascontiguousarray(ranks, dtype=np.int64).ravel()
        count, theta, S = self._draw_range(k0, count, theta)
        lens = self._named_lens(ids, self._widest_site())
        L, R = int(sum(lens)), int(ranks.size)
        out = np.zeros((max(int(count), 0), L, R))
        check(self.lib.epx_named_order_stats(self.ctx, int(k0), int(count), ids.ctypes.data_as(_lib.c_int32_p), len(names),
                                             ranks.ctypes.data_as(_lib.c_int64_p), R, dptr(theta), int(S), dptr(out), None))
        return self._cut_sites(names, lens, out.swapaxes(1, 2), k0, (R,))

    def pooled_count_pass(self, names, shift, prefix, n_targets, k0=0, count=None, theta=None):
        """One counting pass of the pooled selection over the draws of the sites k0..k0+count (epx_pooled_count_pass,
        include/epx.h; quantiles.select_pooled runs the eight passes): (hist (L, n_targets, 256) int64, n_nan (L) int64,
        n), L = the elements of `names` in the order given, which every site of the range has to hold alike.  prefix
        (L, n_targets) uint64, not read at shift 56 (None).  The draws are those of the last sampling call, on the device;
        `theta` (count, S, P) injects draws instead (test hook)."""
        names, ids = self._named_ids(names)
        count, theta, S = self._draw_range(k0, count, theta)
        L, T = int(sum(self._named_lens(ids, k0))), int(n_targets)
        if prefix is not None:
            prefix = np.ascontiguousarray(prefix, dtype=np.uint64)
            if prefix.shape != (L, T):
                raise ValueError('prefix: (L, n_targets) = ({}, {})'.format(L, T))
        hist = np.zeros((L, max(T, 0), 256), dtype=np.int64)
        n_nan = np.zeros(L, dtype=np.int64)
        n = ctypes.c_longlong()
        ll_p = ctypes.POINTER(ctypes.c_longlong)
        check(self.lib.epx_pooled_count_pass(
            self.ctx, int(k0), int(count), ids.ctypes.data_as(_lib.c_int32_p), len(names), int(shift),
            prefix.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if prefix is not None else None, T, dptr(theta), int(S),
            hist.ctypes.data_as(ll_p), n_nan.ctypes.data_as(ll_p), ctypes.byref(n)))
        return hist, n_nan, n.value

    def accept(self, df):
        check(self.lib.epx_accept(self.ctx, float(df)))

    def global_moments(self):
        S = np.empty((self.d, self.d), order='F')
        m = np.empty(self.d)
        check(self.lib.epx_global_moments(self.ctx, dptr(S), dptr(m)))
        return S, m

    def force_pd(self, df, thresh, target):
        forced = np.zeros(self.K, dtype=np.uint8)
        check(self.lib.epx_force_pd(self.ctx, float(df), float(thresh), float(target),
                                    forced.ctypes.data_as(_lib.c_uint8_p)))
        return forced.astype(bool)
