/*
 * epx.h -- C ABI of libepx.so: the MI355X (gfx950) engine behind ep-stan's
 * data-parallel EP inner loop.
 *
 * Every entry point replaces one piece of /root/reference/epstan (cited per
 * function as file:line) and is what a ctypes binding in the reference's
 * epstan/method.py would call instead of PyStan + SciPy/LAPACK (INTEGRATION.md
 * shows that binding).  Conventions:
 *   - extern "C", plain pointers and sizes, no C++/torch types;
 *   - every function returns 0 on success, <0 on error; the message is kept
 *     per thread and read with epx_last_error();
 *   - the caller owns host buffers, the library owns device buffers behind an
 *     opaque epx_ctx bound to ONE HIP device; a ctx is not thread-safe; calls
 *     are synchronous on return (the stream is drained);
 *   - all reals are float64; matrices are column-major ("F order") exactly as
 *     the reference lays them out: site arrays (d,d,K) / (d,K) with the site
 *     index slowest (method.py:838-851), so site k is one contiguous d*d block;
 *   - pointers named *_dev are DEVICE addresses (a caller that runs the reduction between
 *     epx_site_sums() and epx_damped_trial() itself, on device memory of its own);
 *   - several GPUs: one context per rank, bound to the others by epx_comm_init() (RCCL inside
 *     the library); epx_update_trial() then performs the iteration's one all-reduce in stream
 *     order.
 */
#ifndef EPX_H
#define EPX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct epx_ctx epx_ctx;

/* Site log-density families: the reference's single-group Stan programs
 * experiment/models/m{1,2,3,4,5}b_sg.stan (selected by the basename of the
 * `site_model` path given to Master, method.py:647,672). */
enum epx_model { EPX_M1B_SG = 0, EPX_M2B_SG = 1, EPX_M3B_SG = 2, EPX_M4B_SG = 3, EPX_M5B_SG = 4,
                 /* Gaussian-likelihood family, experiment/models/m{1..5}a_sg.stan: phi = [log sigma | the
                  * b-model's phi], y ~ normal(alpha + X beta, sigma), real responses (epx_ctx_create_real) */
                 EPX_M1A_SG = 5, EPX_M2A_SG = 6, EPX_M3A_SG = 7, EPX_M4A_SG = 8, EPX_M5A_SG = 9 };

/* Worker.PREC_ESTIM_OPTIONS, method.py:163 */
enum epx_prec_estim { EPX_PREC_SAMPLE = 0, EPX_PREC_OLSE = 1 };

/* which site array an accessor addresses (method.py:844-851) */
enum epx_which { EPX_QI = 0, EPX_QI2 = 1, EPX_DQI = 2 };

/* init modes of the sampler: Stan's init='random' / '0' (method.py:159, 579-583)
 * or the last draw of each chain of the previous call (init_prev, :404-406). */
enum epx_init { EPX_INIT_RANDOM = 0, EPX_INIT_ZERO = 1, EPX_INIT_PREV = 2 };

/* Sampler settings = Worker.DEFAULT_STAN_PARAMS (method.py:154-160) plus the
 * Stan 2.17 control defaults the reference leaves untouched. */
typedef struct epx_sampler_opts {
    int32_t chains;      /* default 4 */
    int32_t iter;        /* default 1000; fit.py uses 200 */
    int32_t warmup;      /* <0 means iter/2 (warmup=None, method.py:157,567-569) */
    int32_t thin;        /* default 1 */
    int32_t init;        /* enum epx_init */
    int32_t max_depth;   /* Stan max_treedepth, default 10 */
    int32_t layout;      /* 0 auto, 1 one block per site (rows resident in LDS), 2 one block per
                            (site, chain), 3 streaming (rows through an LDS-DMA ring, chains in lock step;
                            chosen automatically when the rows do not fit LDS or D > 32), 4 lock step with
                            the rows resident in LDS (D <= 32; default for multi-group sites), 5 one block per
                            site with a state wave + a row wave per chain (same draws as 1), 6 one block per
                            chain: state wave, two row waves and a bookkeeping wave, 7 one block per site: a state
                            wave per chain + four row waves that serve the site's four chains in lock step on the
                            matrix pipe (v_mfma_f64_4x4x4; the default for batches that fill the chip since
                            round 3; served by 5 when its padded rows do not fit the LDS) */
    int32_t reserved;    /* flags; bit 0: layout 2 without the speculative bookkeeping wave (same draws,
                            used for A/B measurements and tests);
                            bit 1: `adapt = carry` -- NOT the reference's behaviour (a fresh model.sampling per site
                            update re-adapts from scratch, util.py:716), an opt-in the survey sanctions when it is
                            reported: every chain starts from the step size its previous call ended with and from
                            the site's pooled sample variances of that call as diagonal metric (regularised like
                            Stan's estimate), and warm-up adapts the step size only.  Same target distribution;
                            sites without history (first call, a failed chain) adapt from scratch. */
} epx_sampler_opts;

/* per-site sampler statistics written by epx_tilted_batch (doubles) */
enum epx_site_stat {
    EPX_ST_STEPSIZE = 0,   /* mean over chains of mean stepsize__ (method.py:99-102) */
    EPX_ST_RHAT = 1,       /* max split-Rhat over sampled coordinates (method.py:104) */
    EPX_ST_NLEAP = 2,      /* leapfrogs in trees, all chains */
    EPX_ST_NGRAD = 3,      /* gradient evaluations, all chains */
    EPX_ST_NDIV = 4,       /* divergent post-warm-up transitions */
    EPX_ST_ACCEPT = 5,     /* mean post-warm-up accept_stat */
    EPX_ST_DEPTH = 6,      /* mean post-warm-up tree depth */
    EPX_ST_FAIL = 7,       /* >0: a chain started at a non-finite density */
    EPX_ST_COUNT = 8
};

const char *epx_last_error(void);
int epx_device_count(int *count);
/* HIP runtime version (hipRuntimeGetVersion: major * 10^7 + minor * 10^5 + patch) and the device's gcnArchName.  The
 * loader (ep-stan_amd/_lib.py) keys ONE optimisation on them: the piece hand-off without the L2 write-back fence
 * (csrc/epx_pieces.h) is measured behaviour of gfx950 under ROCm 7.2, not an architectural guarantee -- on any other
 * architecture or runtime the loader takes variants/libepx_fence.so (the build with the fence) when it is there.
 * No counterpart in the reference. */
int epx_runtime_info(int device, int *hip_runtime_version, char *arch, int arch_len);
/* Blocks until every stream of `device` is idle (hipDeviceSynchronize).  Every entry point of a context already returns
 * with its own work finished; this is the bracket a measurement harness puts around a timed region (bench.py) without
 * bringing a second HIP runtime -- PyTorch's bundled one -- into the process. */
int epx_device_synchronize(int device);

/* dphi and number of sampled coordinates P of a model (m*b_sg.stan parameter blocks). */
int epx_model_dims(int model, int D, int *dphi, int *npar);

/*
 * Context = the K_local sites of one rank: replaces Master.__init__'s worker
 * construction and array allocation (method.py:817-851).  X is the rank's
 * (N_local, D) row-major block (C-contiguous, method.py:733), y its 0/1
 * responses, k_lim[K_local+1] the row limits of the sites (method.py:700).
 * Sites are ordered; site k owns rows k_lim[k]..k_lim[k+1].
 */
int epx_ctx_create(int device, int model, int K_local, int D, const int64_t *k_lim,
                   const double *X, const int32_t *y, epx_ctx **out);

/* The same for sites that hold SEVERAL groups of the hierarchical model (K < J, experiment/fit.py:310-324:
 * `Master(..., A_k={'J': Nj_k}, A_n={'j_ind': j_ind_k+1})` with the multi-group programs
 * experiment/models/m{1..5}b.stan).  g_cnt[k] = groups in site k; g_lim = row limits of all groups in site
 * order (sum(g_cnt)+1 entries, rank-local rows): the rows of a group are contiguous and the groups of a site
 * tile its rows -- what util.distribute_groups (util.py:582-608) produces.  Site k then samples
 * dphi + g_cnt[k] * (1 [+ D]) coordinates [phi | eta_1.. | etb_1 .. ]; records of draws / last states use the
 * stride of the largest site.  Runs on the streaming sampler layout. */
int epx_ctx_create_groups(int device, int model, int K_local, int D, const int64_t *k_lim, const int32_t *g_cnt,
                          const int64_t *g_lim, const double *X, const int32_t *y, epx_ctx **out);

/* The same for the Gaussian-likelihood models (EPX_M1A_SG..EPX_M5A_SG; `real y[N]` in
 * experiment/models/m1a_sg.stan:16, simulated in models/m1a.py:150-176): y holds real responses.
 * One group per site.  Sites whose rows, cavity precision (and, for one workgroup per chain, the tree stack) fit
 * the LDS run on the resident kernels, all others (D > 32, rows beyond the LDS) on the streaming layout. */
int epx_ctx_create_real(int device, int model, int K_local, int D, const int64_t *k_lim, const double *X,
                        const double *y, epx_ctx **out);
/* ... with several groups per site (experiment/models/m1a.stan:11-45, `j_ind`; g_cnt / g_lim as in
 * epx_ctx_create_groups): the one-workgroup-per-chain layout (D <= 32, <= 128 coordinates), else streaming. */
int epx_ctx_create_real_groups(int device, int model, int K_local, int D, const int64_t *k_lim, const int32_t *g_cnt,
                               const int64_t *g_lim, const double *X, const double *y, epx_ctx **out);
int epx_ctx_destroy(epx_ctx *ctx);

/* prior natural parameters Q0 (d,d) F-order, r0 (d): method.py:772-797 */
int epx_set_prior(epx_ctx *ctx, const double *Q0, const double *r0);

/* host <-> device copies of the site arrays, F-order (d,d,K_local) / (d,K_local)
 * (method.py:844-851); either pointer may be NULL. */
int epx_set_sites(epx_ctx *ctx, int which, const double *QF, const double *rF);
int epx_get_sites(epx_ctx *ctx, int which, double *QF, double *rF);

/* one site's (d,d) / (d) block of a site array: the NumPy views dQi[:,:,k], dri[:,k]
 * that Worker.tilted / Worker.cavity take (method.py:1012-1023, find_damp.py:139,160) */
int epx_set_site(epx_ctx *ctx, int which, int k, const double *Q, const double *r);
int epx_get_site(epx_ctx *ctx, int which, int k, double *Q, double *r);

/* global approximation Q (d,d), r (d) held by the context (method.py:841-842) */
int epx_set_global(epx_ctx *ctx, const double *Q, const double *r);
int epx_get_global(epx_ctx *ctx, double *Q, double *r);

/*
 * Worker.cavity for sites k0..k0+count (method.py:267-302), batched:
 * Mat_k = Q - A_k, vec_k = Mat_k^-1 (r - a_k), posdef[k] = Cholesky succeeded,
 * where (A_k, a_k) = site array `which`; for which == EPX_QI2 the proposal
 * Qi + df*dQi is formed on the fly (method.py:1071-1072) with the df of the
 * last epx_damped_trial.  The results stay on the device as the sampler's
 * Omega_phi / mu_phi (method.py:221-222).
 */
int epx_cavity_batch(epx_ctx *ctx, int which, int k0, int count, uint8_t *posdef);
/* cavity of ONE site from caller-supplied arrays (the find_damp.py:160 pattern) */
int epx_cavity_site(epx_ctx *ctx, int k, const double *Q, const double *r, const double *Qi,
                    const double *ri, uint8_t *posdef);
/* Worker.Mat / Worker.vec of site k after cavity (phase 1) */
int epx_get_cavity(epx_ctx *ctx, int k, double *Mat, double *vec);

/*
 * Worker.tilted for sites k0..k0+count (method.py:305-475), batched: on-GPU
 * NUTS draws from each site's tilted distribution (replaces _sample_stan,
 * method.py:43-118), then mean / scatter / precision estimate / site delta
 * (:410-458) into the device dQi, dri.  seeds[count] are the per-site Stan
 * seeds of method.py:346.  The global (Q, r) subtracted at :457-458 is the one
 * held by the context.  posdef[count] out; stats[count*EPX_ST_COUNT] out (may
 * be NULL); elapsed_ms out (may be NULL): device time of the sampling kernel.
 */
int epx_tilted_batch(epx_ctx *ctx, int k0, int count, const int64_t *seeds,
                     const epx_sampler_opts *opts, int prec_estim, uint8_t *posdef,
                     double *stats, double *elapsed_ms);
/*
 * TEST HOOK: the moment stage alone on injected draws.  samples is
 * (S, d, count) F-order, i.e. per site an (S,d) column-major block like the
 * `samp` array of method.py:362.
 */
int epx_moments_batch(epx_ctx *ctx, int k0, int count, const double *samples, int S,
                      int prec_estim, uint8_t *posdef);
/* Worker.vec (tilted mean) and Worker.Mat (unnormalised scatter C'C) of site k
 * after tilted (phase 2); nsamp out (method.py:408) */
int epx_get_tilted(epx_ctx *ctx, int k, double *Mat, double *vec, int *nsamp);
/*
 * Reuse of the tilted draws across EP iterations (not in the reference).  Between two iterations a site's tilted
 * distribution changes only through its Gaussian cavity, so the tilted moments under the NEW cavity N(mu_n, Om_n^-1) follow
 * from draws sampled against the OLD one N(mu_o, Om_o^-1) by Pareto-smoothed importance sampling, without a likelihood
 * evaluation.  Per site, with the S draws' first d coordinates phi_s and the context's global (Q, r):
 *   1. m0 = (1/S) sum_s phi_s (in the order of the moment stage), c_s = phi_s - m0;
 *   2. dOm = Om_n - Om_o, g = Om_n (mu_n - m0) - Om_o (mu_o - m0), lr_s = g'c_s - c_s'dOm c_s / 2: the log ratio of the
 *      two cavity densities at phi_s up to a constant, centred at m0; identical cavities give lr_s == 0.0 exactly;
 *   3. a lr_s that is not finite: the site's record, mean and scatter are NaN, its flag 0 and dQi = dri = 0;
 *   4. else PSIS as `enum epx_loo` defines it on ll = -lr (tail length, order by (lr, s), Zhang-Stephens fit, cap at 0):
 *      the normalised log weights lw_s, KHAT (+inf exactly when the tail is not smoothed: fewer than 5 tail draws, a
 *      degenerate tail or a non-finite fit; the weights are then the plain normalised ratios), WESS = 1 / sum exp(2 lw_s);
 *   5. w_s = exp(lw_s), dm = sum w_s c_s, tilted mean m0 + dm, n = WESS (a double),
 *      tilted scatter n sum w_s (c_s - dm)(c_s - dm)': with equal weights the mean and scatter of the moment stage;
 *   6. the precision estimate of the moment stage with S replaced by n -- EPX_PREC_SAMPLE: inv(scatter) (n - d - 2),
 *      EPX_PREC_OLSE: on scatter / n with n -- then dQi = Qt - Q, dri = rt - r.  The site fails softly (flag 0, dQi = dri =
 *      0) when the Cholesky fails, and under EPX_PREC_SAMPLE when n - d - 2 <= 0.  nsamp reports S.
 * The results go where epx_tilted_batch leaves them (tilted mean / scatter, dQi, dri, flags, nsamp).
 *
 * epx_set_draw_reuse(ctx, 1): every sampling call from then on keeps a copy of the cavities of the sites it sampled, so
 * that epx_reweight_batch with theta == NULL can reweight the draws of the last sampling call to the context's current
 * cavities.  Off (the default), a sampling call queues nothing extra.
 * epx_reweight_batch: theta == NULL: the draws and the cavity copy of the last sampling call; else theta (count, S, P)
 * row-major with Om_old (count, d, d) column-major and mu_old (count, d), all three required.  The new cavity is the
 * context's current one (epx_cavity_batch / epx_cavity_site / the accepted trial).  posdef[count] out (may be NULL);
 * out: count x EPX_RW_COUNT (may be NULL); elapsed_ms (may be NULL): device time of the kernel.
 */
enum epx_reweight { EPX_RW_KHAT = 0, EPX_RW_WESS, EPX_RW_COUNT };
int epx_set_draw_reuse(epx_ctx *ctx, int on);
int epx_reweight_batch(epx_ctx *ctx, int k0, int count, int prec_estim, const double *theta, int S,
                       const double *Om_old, const double *mu_old, uint8_t *posdef,
                       double *out /* count x EPX_RW_COUNT */, double *elapsed_ms);
/* phi draws of site k in the reference's layout: (S, dphi) F-order, chains
 * concatenated chain-major (util.py:475-484); all sampled coordinates with
 * npar_out = 1: (S, P) F-order. */
int epx_get_draws(epx_ctx *ctx, int k, int all_params, double *out);
int epx_num_draws(epx_ctx *ctx, int *S);

/*
 * Local part of the reduction of method.py:1073-1074:
 * packed = [sum_k Qi (d*d), sum_k ri (d), sum_k dQi (d*d), sum_k dri (d)] over
 * this rank's sites.  Because Q(df) = Q0 + sum Qi + df * sum dQi is affine in
 * df, ONE all-reduce of this buffer per EP iteration serves every damping
 * trial.  Exactly one of packed_host / packed_dev may be non-NULL.
 */
int epx_site_sums(epx_ctx *ctx, double *packed_host, double *packed_dev);
int epx_packed_len(epx_ctx *ctx, int *len);

/*
 * One trial of the damping loop (method.py:1067-1143) with damping factor df:
 * forms Q, r from the (all-reduced) packed sums, Cholesky-checks Q
 * (global_pd), and if positive definite runs the cavities of all local sites
 * against Qi + df*dQi (cav_pd = 1 iff all local cavities are pos.def.,
 * first_bad = first failing local site or -1).
 */
int epx_damped_trial(epx_ctx *ctx, double df, const double *packed_host,
                     const double *packed_dev, int *global_pd, int *cav_pd, int *first_bad);
/* accept: Qi <- Qi + df*dQi, ri <- ri + df*dri (the swap of method.py:1145-1158) */
int epx_accept(epx_ctx *ctx, double df);
/* moments of the accepted global approximation (method.py:1211-1219):
 * S = Q^-1 (d,d), m = S r */
int epx_global_moments(epx_ctx *ctx, double *S, double *m);
/* force-pd fallback, method.py:1119-1129: min eigenvalue of Qi + df*dQi per
 * local site; where it is < thresh, adds (min_eig_target - min_eig) to the
 * diagonal of Qi.  forced[K_local] out. */
int epx_force_pd(epx_ctx *ctx, double df, double thresh, double min_eig_target, uint8_t *forced);

/* Adaptation history of site k kept for `adapt = carry` (written by every sampling call): final step size of
 * each chain (chains entries, -1: none) and the site's diagonal metric (P entries).  Either may be NULL. */
int epx_get_adapt(epx_ctx *ctx, int k, double *eps, double *metric);

/* TEST HOOK: log density and gradient of site k at theta (P) against the
 * cavity currently held for that site (Appendix A of SURVEY.md). */
int epx_logdensity_grad(epx_ctx *ctx, int k, const double *theta, double *lp, double *grad);
/* The same through a chosen sampler layout (epx_sampler_opts.layout; 0 = what a one-site launch would pick):
 * every layout evaluates the density with its own gradient code. */
int epx_logdensity_grad_layout(epx_ctx *ctx, int k, const double *theta, int layout, double *lp, double *grad);
/* TEST HOOK: sampler only (no moment stage) for sites k0..k0+count */
int epx_sample_batch(epx_ctx *ctx, int k0, int count, const int64_t *seeds,
                     const epx_sampler_opts *opts, double *stats, double *elapsed_ms);
/* TEST HOOK: `nt` plain NUTS transitions (no adaptation) per (site, chain) from
 * given positions q0 (count, chains, P) with given step sizes eps (count, chains)
 * and diagonal inverse metrics inv_e (count, chains, P); the random stream is the
 * one a full run uses at transitions t_offset, t_offset+1, ...  q_out is
 * (count, chains, nt, P), chain_stats (count, chains, EPX_ST_COUNT). */
int epx_nuts_transitions(epx_ctx *ctx, int k0, int count, const int64_t *seeds, int chains, int nt,
                         int t_offset, int layout, const double *q0, const double *eps,
                         const double *inv_e, double *q_out, double *chain_stats);
/* chain stats of the last sampling call: (count, chains, EPX_ST_COUNT) */
/* Sums for Master.mix_phi (method.py:1250-1296, the posterior approximation from the pooled tilted
 * samples): out = [sum_k scatter_k (d*d, column-major), sum_k mean_k (d), sum_k mean_k mean_k' (d*d)] over this
 * context's sites, from the tilted moments of the last epx_tilted_batch / epx_moments_batch. */
int epx_mix_sums(epx_ctx *ctx, double *out);

/* Named parameters of the site models for Master.mix_pred (method.py:1304-1478, called by experiment/fit.py:408-421 with
 * the models' inferred parameters `alpha`, `beta`): the reference walks `worker.fit.extract(pars=par)` of every worker on
 * the host; here the draws of every sampled coordinate theta = [phi | eta (groups) | etb (groups x D)] are still in device
 * memory when a sampling call returns, and the `parameters` / `transformed parameters` of
 * experiment/models/m{1..5}{a,b}[_sg].stan are applied to them there:
 *   phi eta etb mu_a mu_b: coordinates;  sigma_a sigma_b sigma: exp of their logarithms in phi;
 *   alpha = [mu_a +] eta sigma_a;  beta = [mu_b +] etb sigma_b (element-wise), m1b: phi's `beta` slice. */
enum epx_named { EPX_NM_PHI = 0, EPX_NM_ETA, EPX_NM_ALPHA, EPX_NM_BETA, EPX_NM_SIGMA_A, EPX_NM_ETB, EPX_NM_SIGMA_B,
                 EPX_NM_MU_A, EPX_NM_MU_B, EPX_NM_SIGMA, EPX_NM_COUNT };
/* elements of `name` at site k (its per-site shape flattened in C order: (ng,), (ng, D), (D,), (d,), scalars 1);
 * error if the context's model does not define the name */
int epx_named_len(epx_ctx *ctx, int k, int name, int *len);
/* Per site and element the mean and the CENTRED sum of squares M2 = sum_s (x_s - mean)^2 over the site's draws (two
 * passes; what method.py:1390-1395 / :1426-1430 compute per worker): mean[count * L], m2[count * L], L = sum over the
 * names of the length at the context's LARGEST site; row = site, names in the order given (at most 16), zero behind a
 * site's own elements.  theta == NULL: the draws of the last sampling call (error "no draws yet" before one, and an
 * error when that call did not cover every site of the range: their draws would be stale), S is ignored; otherwise TEST HOOK: injected draws (count, S, P) row-major, P = the context's record stride (a site reads
 * its own coordinates of a row only).  nsamp out (may be NULL): draws per site.  One launch, one synchronisation. */
int epx_named_moments(epx_ctx *ctx, int k0, int count, const int32_t *names, int n_names,
                      const double *theta, int S, double *mean, double *m2, int *nsamp);

/* Moments of the phi draws of the sites k0..k0+count POOLED: what the consensus run forms from the concatenated draws of
 * all its sites (experiment/fit.py:639-646, `samp = np.concatenate(samples)`, and the `TODO make more efficient` there),
 * taken from the draws where they lie in device memory.  Over all n = count * draws-per-site draws x:
 *   sum[i] = sum (x_i - center_i),  scatter = sum (x - center)(x - center)' (d*d column-major, both triangles),
 * d = dphi: only the first d coordinates of a draw record take part; the record stride is the context's P (in
 * multi-group contexts the stride of the largest site; nothing behind a record's first d coordinates is read).
 * center == NULL: 0.  want_scatter == 0: the sums alone, scatter may be NULL.  n out: the number of draws.
 * theta == NULL: the draws of the last sampling call (error "no draws yet" before one, and an error when that call did
 * not cover every site of the range), S is ignored; otherwise TEST HOOK: injected draws (count, S, P) row-major as
 * epx_named_moments takes them.  No per-site factorisation and no S >= d requirement; the site arrays, the tilted
 * moments and dQi / dri are neither read nor written.  Partial 16 x 16 tiles per slab of draws go to a workspace of the
 * context and are added in a fixed order (no floating-point atomics): the same bits on every call.  Stream-ordered, one
 * synchronisation. */
int epx_pooled_moments(epx_ctx *ctx, int k0, int count, const double *center /* d, or NULL = 0 */,
                       const double *theta, int S, int want_scatter,
                       double *sum /* d */, double *scatter /* d*d column-major, may be NULL */, long long *n);

/* Posterior predictive of NEW rows from the draws of the sites k0..k0+count (no counterpart in the reference, whose user
 * extracts every draw and re-applies the models' `transformed parameters` by hand).  For a new row x_i in group g of a
 * site and every draw s of that site, f_si = alpha_g(s) + x_i . beta_g(s), with alpha and beta as EPX_NM_ALPHA /
 * EPX_NM_BETA above form them.  Per row, over the site's S draws:
 *   EPX_PR_MEAN    (1/S) sum_s sigmoid(f_si) for the Bernoulli-logit models, (1/S) sum_s f_si for the Gaussian ones;
 *   EPX_PR_F_MEAN  (1/S) sum_s f_si;
 *   EPX_PR_F_M2    sum_s (f_si - F_MEAN)^2, centred, in a second pass;
 *   EPX_PR_LPD     log (1/S) sum_s exp(ll_si) with ll = y f - log(1 + e^f), or the logarithm of the normal density of y at
 *                  mean f and scale exp(phi_s[0]); a log-mean-exp about the row's largest ll; NaN when yn == NULL.
 * The rows are given by site: those of site k0 + j are [row_lim[j], row_lim[j+1]), row_lim[0] = 0, n = row_lim[count];
 * a site or a group may have none, n == 0 returns without a launch.  row_group: 0-based group within the row's site, in
 * any order (NULL: group 0 everywhere).  Xn (n x D row-major), yn (n; 0 or 1 for the Bernoulli models) and out
 * (n x EPX_PR_COUNT row-major) are host arrays.  theta == NULL: the draws of the last sampling call (error "no draws
 * yet" before one, and an error when that call did not cover every site of the range), S is ignored; otherwise TEST HOOK:
 * injected draws (count, S, P) row-major as epx_named_moments takes them (a site reads its own coordinates of a record
 * only).  nsamp out (may be NULL): draws per site.  At most D = 128 columns.  No floating-point atomics: the same bits
 * on every call.  Stream-ordered, one launch, one synchronisation. */
enum epx_pred { EPX_PR_MEAN = 0, EPX_PR_F_MEAN, EPX_PR_F_M2, EPX_PR_LPD, EPX_PR_COUNT };
int epx_predict(epx_ctx *ctx, int k0, int count, const int64_t *row_lim, const int32_t *row_group, const double *Xn,
                const double *yn, const double *theta, int S, double *out, int *nsamp);

/* Posterior predictive of a group that was NOT in the data (no counterpart in the reference): the new group's own latents
 * are drawn from the model's prior on the device and the pool of all sites' phi draws is pushed through them.  The
 * definition, stated once; the kernels (csrc/newgroup.inc) and newgroup.predict_new_group_host both follow it.
 * Pool.  The sites k0..k0+count hold S draws each; only the first d = dphi coordinates phi of a draw record are read
 *   (record stride P: multi-group contexts are fine).  Every draw is used with R >= 1 independent replicates of the new
 *   group's latents: a pool member is (b, s, r), b < count, s < S, r < R, N = count S R of them.  The pooled draw index is
 *   t = t0 + b S + s, t0 being the index of site k0's first draw among ALL sites of ALL ranks (Master passes
 *   (k_lo + k0) S: results do not depend on how the sites are sharded); t0 + count S <= 2^32.
 * Latents of new group `label` (0 <= label < 2^31) at (t, r): E = 1 + D elements for the models with an etb block
 *   (m2..m5), E = 1 for m1; element e = 0 is eta, e = 1 + j is etb_j.  With (u1, u2) the two uniforms of the samplers'
 *   Philox4x32-10 stream at key (seed, chain = label) and counter (t, kind 6 = K_NEWGROUP, e >> 1, r) -- a kind no sampler
 *   uses -- m1..m4 (eta, etb ~ normal(0, 1)) take the Box-Muller pair shared by e and e ^ 1,
 *   z_e = sqrt(-2 log u1) cos(2 pi u2) for even e, ... sin ... for odd e; m5 (double_exponential(0, 1)) takes u = u2 for
 *   odd e, else u1, x = u - 1/2, z_e = -sign(x) log1p(-2 |x|).  u lies in the open interval: z_e is finite.  A latent
 *   depends on (seed, label, t, r, e) only.
 * Coefficients.  alpha_n, beta_n as EPX_NM_ALPHA / EPX_NM_BETA form them, with eta := z_0, etb_j := z_{1+j} (m1 takes
 *   beta from phi); f_{n,i} = alpha_n + x_i . beta_n; link and ll_{n,i} as in EPX_PR_LPD above.
 * Per row i, over the N pool members: the four columns of enum epx_pred with S read as N (F_M2 centred, LPD a
 *   log-mean-exp about the largest term, NaN when yn == NULL).
 * Per new group g with rows I_g: EPX_NG_GLPD = log (1/N) sum_n exp(sum_{i in I_g} ll_{n,i}), the joint log predictive
 *   density of the group's responses -- all rows of the group share the member's latents; a log-mean-exp about the
 *   largest sum, finite where every term underflows; 0 for a group without rows; NaN when yn == NULL.
 * Merging two disjoint pools a, b (chunks of the pool inside the call; ranks, on the host: newgroup.merge):
 *   the means by weights; M2 = M2_a + M2_b + (fmean_a - fmean_b)^2 N_a N_b / N;
 *   lpd = logaddexp(lpd_a + log N_a, lpd_b + log N_b) - log N, taken about the larger term; GLPD like lpd.
 * Results, never faults: log sigma = -800 gives exp = 0 and the latents drop out; non-finite phi gives what the
 * arithmetic gives, for the rows and groups it touches only.
 * Xn (n x D row-major), yn (n; 0 or 1 for the Bernoulli models, finite for the Gaussian ones; or NULL), row_group (n:
 * dense index 0..G-1 of the row's new group, any order; NULL: all 0), group_label (G), out (n x EPX_PR_COUNT) and out_group
 * (G x EPX_NG_COUNT, may be NULL) are host arrays; N out (may be NULL): the pool's members.  n == 0 returns N without a
 * launch and writes neither out nor out_group.  theta == NULL: the draws of the last sampling call (error "no draws yet"
 * before one, and an error when that call did not cover every site of the range), S is ignored; otherwise TEST HOOK:
 * injected draws (count, S, P) row-major.  1 <= R <= 1024, at most D = 128 columns.  The pool is cut into chunks of whole
 * slabs of 16 members by a rule that depends on N alone; chunk records go to a workspace of the context and are merged in
 * ascending order.  No floating-point atomics: the same bits on every call, and the bits of a row's record or of a
 * group's GLPD do not depend on which other rows or groups are in the call.  Stream-ordered, one synchronisation. */
enum epx_newgroup { EPX_NG_GLPD = 0, EPX_NG_COUNT };
int epx_predict_new_group(epx_ctx *ctx, int k0, int count, uint64_t seed, long long t0, int R,
                          long long n, const double *Xn /* n x D */, const double *yn /* n or NULL */,
                          const int32_t *row_group /* n, dense 0..G-1, or NULL: all 0 */,
                          int G, const int32_t *group_label /* G: the stream's label of each group */,
                          const double *theta, int S,          /* NULL: last sampling call; else TEST HOOK (count,S,P) */
                          double *out /* n x EPX_PR_COUNT */, double *out_group /* G x EPX_NG_COUNT, may be NULL */,
                          long long *N);
/* TEST HOOK, no context: latents of `label` at pooled draws t0..t0+nt, replicates 0..R: out (nt, R, E) */
int epx_newgroup_latents(int device, int model, int D, uint64_t seed, int32_t label, long long t0,
                         long long nt, int R, double *out);

/* Leave-one-out cross-validation of the context's OWN rows from the draws of the sites k0..k0+count: PSIS-LOO (Pareto-
 * smoothed importance sampling) with its Pareto k-hat diagnostic, and what WAIC needs (no counterpart in the reference).
 * The definition, stated once; the kernels k_loo / k_psis_rows (csrc/predict.hip, csrc/psis.h) and loo.psis_host /
 * loo.loo_host both follow it.  For a training row i of site k, ll_s is the log-likelihood of its response under draw s of
 * that site: EPX_PR_LPD's ll, with f_si = alpha_g(s) + x_i . beta_g(s), alpha and beta as EPX_NM_ALPHA / EPX_NM_BETA form
 * them, ll = y f - log(1 + e^f) or the logarithm of the normal density of y at mean f and scale sigma = exp(phi_s[0]).
 * Per row, over the site's S draws:
 *   EPX_LO_LPD      log (1/S) sum_s exp(ll_s), a log-mean-exp about the largest term: EPX_PR_LPD of the row;
 *   EPX_LO_LL_MEAN  (1/S) sum_s ll_s;
 *   EPX_LO_LL_M2    sum_s (ll_s - LL_MEAN)^2, centred, in a second pass (the row's WAIC penalty is LL_M2 / (S - 1));
 *   EPX_LO_ELPD, EPX_LO_KHAT, EPX_LO_WESS   PSIS:
 *     1. lr_s = -ll_s - max_s(-ll_s): the largest is 0.
 *     2. M = min(floor(S / 5), ceil(3 sqrt(S))).
 *     3. The draws are ordered by (lr_s, s) ascending (ties go by draw index); the tail is the last M, u the value in
 *        front of it.
 *     4. Excesses x_j = exp(lr_tail_j) - exp(u), j = 1..M, ascending.
 *     5. If M >= 5, x_q > 0 with q = floor(M / 4 + 0.5) (1-based) and x_M > x_q, a generalised Pareto distribution is
 *        fitted by Zhang & Stephens: m = 30 + floor(sqrt(M)); b_i = 1 / x_M + (1 - sqrt(m / (i - 0.5))) / (3 x_q),
 *        i = 1..m; k_i = mean_j log1p(-b_i x_j); L_i = M (log(-b_i / k_i) - k_i - 1); w_i = 1 / sum_j exp(L_j - L_i);
 *        b = sum_i b_i w_i; k = mean_j log1p(-b x_j); sigma = -k / b; KHAT = (M k + 5) / (M + 10) (the weakly
 *        informative prior: ten pseudo-observations at 0.5).
 *     6. If KHAT is finite, the tail's lr are replaced in rank order by min(0, log(exp(u) + q_j)),
 *        q_j = (sigma / KHAT) expm1(-KHAT log1p(-p_j)), p_j = (j - 0.5) / M; at KHAT = 0, q_j = -sigma log1p(-p_j).
 *     7. lw = lr - logsumexp(lr).
 *     8. ELPD = logsumexp(lw + ll).
 *     9. WESS = 1 / sum_s exp(2 lw_s).
 * Results, never faults: when a condition of step 5 fails or KHAT comes out non-finite nothing is smoothed, KHAT = +inf
 * and ELPD, WESS come from the raw ratios; a row with any non-finite ll_s has NaN in all six; S = 1 gives LL_M2 = 0.
 * out (host): rows x EPX_LO_COUNT row-major for the rows k_lim[k0] .. k_lim[k0 + count] in the context's row order.  The
 * rows, the responses and the group limits are the context's: nothing is uploaded but the work list.  theta == NULL: the
 * draws of the last sampling call (error "no draws yet" before one, and an error when that call did not cover every site
 * of the range), S is ignored; otherwise TEST HOOK: injected draws (count, S, P) row-major as epx_named_moments takes
 * them (a site reads its own coordinates of a record only).  nsamp out (may be NULL): draws per site.  At most D = 128
 * columns.  A tile's 16 x S log-likelihoods are kept in LDS while they fit (about 900 draws at D = 32; the environment variable
 * EPX_LOO_LDS_BYTES, read at every call, lowers the budget, for A/B runs and tests; a value that is no whole non-negative
 * number is ignored, as for EPX_PO_LDS_BYTES); longer runs keep them in a workspace sized by the grid:
 * the same bits.  The tail, its candidates and the fit need about 16 (2.5 M + 106) doubles of LDS: an S beyond that (about 20000) is an error.  No
 * floating-point atomics: the same bits on every call.  Stream-ordered, one launch, one synchronisation. */
enum epx_loo { EPX_LO_LPD = 0, EPX_LO_LL_MEAN, EPX_LO_LL_M2, EPX_LO_ELPD, EPX_LO_KHAT, EPX_LO_WESS, EPX_LO_COUNT };
int epx_loo(epx_ctx *ctx, int k0, int count, const double *theta, int S, double *out /* rows x EPX_LO_COUNT */, int *nsamp);

/* The PSIS stage alone (steps 1..9 above, the same device code) on log-likelihoods the caller gives: ll (n x S row-major,
 * host) -> out (n x 3, host: ELPD, KHAT, WESS); NaN in all three for a row with a non-finite entry.  Needs no context and
 * leaves the calling thread's current device as it found it. */
int epx_psis_rows(int device, long long n, int S, const double *ll, double *out /* n x 3 */);

/* Posterior predictive checks of the context's OWN rows from the draws of the sites k0..k0+count (no counterpart in the
 * reference): the responses are replicated from every draw on the device and a statistic of the replicated data is
 * compared with the same statistic of the observed data, group by group.  The definition, stated once; the kernels k_ppc /
 * k_ppc_sites (csrc/ppc.inc) and ppc.ppc_host both follow it.
 * A GROUP is one (site, group within the site) of the context's rows; for an `_sg` model it is the site.  For group g with
 * rows i in g and draw s of its site, f_is = alpha_g(s) + x_i . beta_g(s), alpha and beta as EPX_NM_ALPHA / EPX_NM_BETA
 * form them (EPX_PR_LPD's f).
 * Replicates.  One per (row, draw), from the samplers' Philox4x32-10 stream at key (seed, chain = 0) and kind 7 = K_PPC --
 * a kind no sampler uses.  `row` is the context's row index plus row0 (Master passes the index of this rank's first row
 * among ALL rows: results do not depend on how the sites are sharded); 0 <= row0 and row0 + k_lim[k0 + count] < 2^32.
 *   Bernoulli-logit family: y_rep_is = 1 if u1 < sigmoid(f_is), else 0, u1 the first uniform of counter (s, K_PPC, row, 0).
 *   Gaussian family: y_rep_is = f_is + sigma_s z, sigma_s = exp(phi_s[0]), z the standard normal of vector element e = row
 *   of the samplers' stream: with (u1, u2) the uniforms of counter (s, K_PPC, e >> 1, 0), e the row as a 32-bit signed
 *   integer, z = sqrt(-2 log u1) cos(2 pi u2) for even e, ... sin ... for odd e.
 *   A replicate depends on (seed, row, s) only: not on the sites of the call, the number of ranks or the launch grid.
 * Per (group, draw), with ll the log-likelihood term of EPX_PR_LPD (y f - log(1 + e^f), or the logarithm of the normal
 * density at mean f and scale sigma_s):
 *   T_rep_s = sum_i y_rep_is;  D_obs_s = sum_i ll(y_i | s);  D_rep_s = sum_i ll(y_rep_is | s);  per group T_obs = sum_i y_i.
 *   D is the realised discrepancy of Gelman, Meng & Stern: for the Gaussian family it compares sum ((y - f) / sigma)^2 with
 *   a chi-square on n_g degrees of freedom, for the Bernoulli family the deviance of the observed responses with that of
 *   replicated ones.  D_obs_s and D_rep_s are added over the same rows in the same order: where y_rep = y on every row of
 *   the group they are equal to the bit.
 * The record of a unit, over the S draws:
 *   EPX_PC_T_OBS       T_obs;
 *   EPX_PC_T_MEAN      (sum_s T_rep_s) / S;
 *   EPX_PC_T_M2        sum_s (T_rep_s - T_MEAN)^2, centred, in a second pass;
 *   EPX_PC_T_GE, EPX_PC_T_GT   the number of draws with T_rep_s >= T_obs, with T_rep_s > T_obs;
 *   EPX_PC_D_OBS_MEAN, EPX_PC_D_REP_MEAN   (sum_s D_obs_s) / S, (sum_s D_rep_s) / S;
 *   EPX_PC_D_LE        the number of draws with D_rep_s <= D_obs_s.
 *   The three counts are integers held in doubles; the host turns them into p-values (ppc.summarise).
 * A unit is a group, or a SITE: a site's per-draw values are the sums of its groups' per-draw values, added in group
 * order, its T_obs likewise; for an `_sg` model the site's record repeats its one group's.  There is no total over sites:
 * a statistic that pairs draw s of different sites has no meaning.
 * Results, never faults: a group with a non-finite f, ll(y) or ll(y_rep) in any cell has NaN in all eight columns, and so
 * has the site that contains it.
 * out_groups (host, required): groups of the range x EPX_PC_COUNT row-major, in the context's order; out_sites (host, may
 * be NULL): count x EPX_PC_COUNT; out_draws (host, may be NULL): groups x 3 x S, the per-draw T_rep, D_obs, D_rep of every
 * group.  The rows, the responses and the group limits are the context's: nothing is uploaded but the work list.
 * theta == NULL: the draws of the last sampling call (error "no draws yet" before one, and an error when that call did not
 * cover every site of the range), S is ignored; otherwise TEST HOOK: injected draws (count, S, P) row-major as
 * epx_named_moments takes them.  nsamp out (may be NULL): draws per site.  At most D = 128 columns and 2^31 - 1 rows.  A
 * group's 3 x S per-draw sums are kept in LDS: an S beyond (160 KiB - 1 KiB - the fixed part) / 24 bytes (about 6500 at
 * D = 32) is an error that names S and the limit; there is no fallback.  No floating-point atomics and nothing merged
 * across workgroups: the same bits on every call, whatever the grid and whichever other sites are in the call.
 * Stream-ordered, two launches, one synchronisation. */
enum epx_ppc { EPX_PC_T_OBS = 0, EPX_PC_T_MEAN, EPX_PC_T_M2, EPX_PC_T_GE, EPX_PC_T_GT, EPX_PC_D_OBS_MEAN,
               EPX_PC_D_REP_MEAN, EPX_PC_D_LE, EPX_PC_COUNT };
int epx_ppc(epx_ctx *ctx, int k0, int count, uint64_t seed, long long row0, const double *theta, int S,
            double *out_groups /* groups x EPX_PC_COUNT */, double *out_sites /* count x EPX_PC_COUNT, may be NULL */,
            double *out_draws /* groups x 3 x S, may be NULL */, int *nsamp);

/* Predictive intervals of NEW rows: order statistics across the draws of every row's linear predictor or replicated
 * response (no counterpart in the reference, whose user calls `fit.extract`, re-applies alpha + x . beta by hand and calls
 * np.percentile).  The definition, stated once; the kernel k_predict_order (csrc/predict_order.inc) and
 * predict_quantiles.predict_order_stats_host both follow it.
 * The new rows are described exactly as epx_predict takes them: sorted by site, those of site k0 + j are
 * [row_lim[j], row_lim[j+1]), row_lim[0] = 0, n = row_lim[count]; row_group: 0-based group within the row's site (NULL:
 * group 0 everywhere).  For row i of site k and draw s of that site, f_is is EPX_PR_F_MEAN's f = alpha_g(s) + x_i . beta_g(s),
 * alpha and beta as EPX_NM_ALPHA / EPX_NM_BETA form them.  `what` selects the value v_is that is ordered:
 *   EPX_PO_F     v_is = f_is; both families.
 *   EPX_PO_YREP  v_is = f_is + sigma_s z, sigma_s = exp(phi_s[0]): the replicated response.  Gaussian family only; a
 *                Bernoulli-logit model is an error that says so (a 0/1 replicate has no useful quantile).  z is built exactly
 *                as epx_ppc builds its Gaussian replicate, at the stream kind 9 = K_PRED_REP, which no sampler uses: key
 *                (seed, chain = 0), with (u1, u2) the uniforms of counter (s, K_PRED_REP, e >> 1, 0), e as a 32-bit signed
 *                integer, z = sqrt(-2 log u1) cos(2 pi u2) for even e, ... sin ... for odd e.  e = row_id[i], the caller's
 *                stream index of the row in [0, 2^32) (outside: an error); row_id == NULL: e = i, the row's position in the
 *                call.  A replicate depends on (seed, row_id, s) only: not on the sites of the call, the row order, the
 *                ranks or the grid.  EPX_PO_F checks row_id's range all the same and uses neither it nor seed.
 * Per row the n_ranks order statistics v_(ranks[r]) of its S values: the draws ordered by the key of "Posterior quantiles"
 * below, ranks ascending, distinct, in [0, S), between 1 and 32 (EPX_QT_MAX_RANKS).  A row with a NaN among its v_is has
 * NaN at every rank, that row alone; +-inf are ordinary values.  out (host): n x n_ranks row-major, the caller's row order.
 * The HOST interpolates (quantiles.rank_plan, quantiles.interpolate), as for epx_named_order_stats.
 * theta == NULL: the draws of the last sampling call (error "no draws yet" before one, and an error when that call did not
 * cover every site of the range), S is ignored; otherwise TEST HOOK: injected draws (count, S, P) row-major as
 * epx_named_moments takes them.  nsamp out (may be NULL): draws per site.  At most D = 128 columns and 2^31 - 1 rows; n == 0
 * returns without a launch.  A refusal launches nothing and writes nothing.
 * Draw limit.  A workgroup takes work items of up to R rows of one (site, group), cut as epx_predict cuts its own, and sorts
 * the item's keys in LDS, every row padded to N(S) = S rounded up to a power of two (at least 2) with the all-ones key.  R
 * is the largest of 16, 8, 4, 2, 1 for which R x N(S) x 8 bytes fit the budget: 160 KiB - 1 KiB - the walk's fixed part (four
 * coefficient slabs of 16 x (1 + D rounded up to 4) doubles, one per wave, each with 32 doubles of scales, and 8 doubles of
 * NaN flags: 19 520 bytes at D = 32).  When not even
 * R = 1 fits the call is an error that names S and the largest admissible S; there is no workspace fallback.  At D = 32:
 * R = 16 up to S = 1024, at most S = 16384.  The environment variable EPX_PO_LDS_BYTES, read at every call, replaces the
 * budget where it is smaller (tests reach R < 16 and the limit at small S with it; a value that is no whole non-negative
 * number is ignored, and a refusal under a lowered budget names the variable); results do not depend on R.
 * No floating-point atomics, no atomics at all, nothing merged across workgroups: a row's result has the same bits on every
 * call, whatever the grid, the sub-range of sites or the other rows of the call.  Stream-ordered, one launch, one
 * synchronisation. */
enum epx_pred_order { EPX_PO_F = 0, EPX_PO_YREP = 1 };
int epx_predict_order_stats(epx_ctx *ctx, int k0, int count, const int64_t *row_lim, const int32_t *row_group,
                            const double *Xn, const int64_t *row_id /* n, or NULL */, int what, uint64_t seed,
                            const int64_t *ranks, int n_ranks, const double *theta, int S,
                            double *out /* n x n_ranks */, int *nsamp);

/* The site normaliser of EP, log Z_k, by bridge sampling on the device (no counterpart in the reference, which has no
 * evidence estimate).  The definition, stated once; the kernels k_ev_fit / k_ev_bridge (csrc/evidence.hip), k_ev_terms
 * (csrc/evidence_terms.inc) and evidence.site_evidence_host all follow it.  What is estimated per site is log int exp(lq), lq the UNNORMALISED log
 * density the site's sampler draws from; evidence.site_log_z and evidence.combine turn the sites' values into log Z_EP.
 * Draws and cavity.  Site k has P_k sampled coordinates theta = [phi (d) | lambda], lambda = eta per group, then etb per
 *   group x D, as epx_named_moments lays them out (P_k = P for a single-group context; a multi-group site uses its own
 *   d + groups x (1 or 1 + D) coordinates).  Its S draws come in the device's order, chain-major: `chains` chains of
 *   n = S / chains draws.  Its cavity (mu, Omega) is the context's current one (epx_get_cavity).
 * Split.  The fit set F is the first floor(n / 2) draws of every chain, the estimation set E the rest, both in the
 *   device's order; N1 = |E|, N2 = N1.
 * Proposal.  m = the mean over F; C = the centred scatter over F / (|F| - 1), from a second pass (never sum theta theta'
 *   - n m m'); L = the lower Cholesky factor of C.
 * Proposal draws.  theta~_r = m + L z_r, r < N2, z_{r,e} the standard normal of element e of the samplers' Philox4x32-10
 *   stream at key (seed, chain = site0 + k), k the site's index in the context, counter (r, kind 8 = K_BRIDGE, e >> 1, 0):
 *   with (u1, u2) its uniforms, z = sqrt(-2 log u1) cos(2 pi u2) for even e, ... sin ... for odd e (epx_predict_new_group
 *   states the same pair).  site0 is the index of the context's first site among ALL sites of all ranks, 0 <= site0 and
 *   site0 + K < 2^31: a site's record does not depend on the sharding.
 * Target.  lq(theta) = -1/2 (phi - mu)' Omega (phi - mu) + lprior(lambda) + sum_{i in site} ll_i(theta), lprior =
 *   -1/2 |lambda|^2 (m1..m4) or -|lambda|_1 (m5), ll_i the log-likelihood term of EPX_PR_LPD with f from EPX_NM_ALPHA /
 *   EPX_NM_BETA of the row's group.  Logistic family: lq is the sampler's lp.  Gaussian family: the sampler's lp minus
 *   n_k 1/2 log 2 pi (the sampler drops that constant, EPX_PR_LPD keeps it).
 * Proposal density.  lg(theta) = -1/2 |L^-1 (theta - m)|^2 - sum log L_ii - (P_k / 2) log 2 pi; for a proposal draw the
 *   quadratic form is |z_r|^2 taken from z itself.
 * Terms.  l1_s = lq(theta_s) - lg(theta_s), s in E;  l2_r = lq(theta~_r) - lg(theta~_r).
 * Bridge (Meng & Wong's optimal bridge), in log space: s1 = N1 / (N1 + N2), s2 = N2 / (N1 + N2), LSE2(a, b) = t +
 *   log(e^(a - t) + e^(b - t)) about t = max(a, b);
 *     rho_0 = LSE_r(l2_r) - log N2
 *     rho_{t+1} = [LSE_r(l2_r - LSE2(log s1 + l2_r, log s2 + rho_t)) - log N2]
 *               - [LSE_s(-LSE2(log s1 + l1_s, log s2 + rho_t)) - log N1]
 *   every LSE about its largest term, every sum in a fixed order; stop when |rho_{t+1} - rho_t| <= 1e-10 or after 1000
 *   iterations.
 * The record of a site:
 *   EPX_EV_LOGZ      the final rho: log int exp(lq);
 *   EPX_EV_LOGZ_IS   rho_0, the plain importance-sampling estimate from the proposal draws;
 *   EPX_EV_ITERS     iterations used; 1001: not converged;
 *   EPX_EV_RE2       Var(f2) / (N2 mean(f2)^2) + Var(f1) / (N1 mean(f1)^2), f1_s = 1 / (s1 e^(l1_s - rho) + s2), f2_r =
 *                    e^(l2_r - rho) / (s1 e^(l2_r - rho) + s2), Var with divisor N - 1, centred in a second pass: the relative
 *                    mean-square error of e^rho that treats the draws of both sets as INDEPENDENT.  The chains'
 *                    autocorrelation is not in it: with an effective sample size below N1 the true error is larger;
 *   EPX_EV_KHAT      the PSIS k-hat of the proposal's importance ratios e^(l2): steps 1-5 of enum epx_loo on ll = -l2 (the
 *                    same code, psis.h); +inf where the tail is not fitted;
 *   EPX_EV_N1        N1.
 * Results, never faults: a site with a non-finite l1 or l2, or whose Cholesky factorisation meets a pivot that is not
 *   finite or numerically <= 0 -- at most P_k 2^-50 C_jj, what rounding alone leaves of an exact zero (a non-finite draw
 *   in F, a duplicated coordinate) --, has NaN in LOGZ, LOGZ_IS, RE2 and KHAT and 0 in ITERS;
 *   the other sites of the call are unaffected.
 * Refusals, known from sizes alone, before any launch, each naming its numbers: D > 128; a P whose packed factor and
 *   workspace do not fit the LDS (epx_kernels.h: evidence_max_coords, 166 at D = 32, so m4b's P = 99 is admitted; no
 *   fallback); chains that do not divide S; |F| < 2 P; an N1 whose terms do not fit the LDS of the bridge.
 * out (host, required): count x EPX_EV_COUNT.  out_terms (host, may be NULL; the tests read it): per site
 *   [l1 (N1) | l2 (N1) | m (P) | L packed by rows, L_ij at i (i + 1) / 2 + j (P (P + 1) / 2) | theta~ (N2 x P)], zeros
 *   behind a multi-group site's own P_k; without it the proposal draws never leave the chip.
 * theta == NULL: the draws of the last sampling call and its chains (error "no draws yet" before one, and an error when
 *   that call did not cover every site of the range), S is ignored, and chains is 0 or -- from a caller that sized
 *   out_terms by it -- the chains of that call: any other value is an error; otherwise TEST HOOK: injected draws
 *   (count, S, P) row-major, chain-major, with their `chains`.  No floating-point atomics, nothing merged across
 *   workgroups: the same bits on every call, whichever other sites are in the call.  Stream-ordered, three launches, one
 *   synchronisation; elapsed_ms (may be NULL): the device time of the three. */
enum epx_evidence { EPX_EV_LOGZ = 0, EPX_EV_LOGZ_IS, EPX_EV_ITERS, EPX_EV_RE2, EPX_EV_KHAT, EPX_EV_N1, EPX_EV_COUNT };
int epx_site_evidence(epx_ctx *ctx, int k0, int count, uint64_t seed, long long site0, const double *theta, int S,
                      int chains, double *out /* count x EPX_EV_COUNT */, double *out_terms /* may be NULL */,
                      double *elapsed_ms);

/* Per-coordinate diagnostics of the draws of the sites k0..k0+count (no counterpart in the reference, which reports the
 * largest split-Rhat of a site and nothing else: EPX_ST_RHAT above stays as it is).  The definition, stated once; the
 * kernel k_draw_diag and diagnostics.diagnostics_host both follow it.  Per site and per sampled coordinate x: every chain
 * is split into its first and its last h = nkeep / 2 draws (an odd nkeep drops the middle draw), M = 2 chains half chains
 * of length h, n = M h used draws.  With mean_m the mean of half chain m, dev = x - mean_m (centred in a second pass) and
 * acov_m(t) = (1/h) sum_{i < h-t} dev_i dev_{i+t}:
 *   W        = mean_m acov_m(0) h / (h - 1)
 *   var_plus = W (h - 1) / h + var(mean_m, ddof = 1)
 *   rho(t)   = 1 - (W - mean_m acov_m(t)) / var_plus
 *   EPX_DG_MEAN    mean_m mean_m;
 *   EPX_DG_VAR     var_plus;
 *   EPX_DG_RHAT    sqrt(var_plus / W): split-Rhat, algebraically what EPX_ST_RHAT takes the maximum of;
 *   EPX_DG_ESS     n / tau, with Geyer's initial positive, monotone sequence over pairs of lags: pair_0 = 1 + rho(1),
 *                  pair_j = rho(2j) + rho(2j+1) while 2j+1 < h, ended in front of the first pair that is not > 0, every
 *                  pair replaced by the smallest pair so far, tau = -1 + 2 sum pairs, floored at 1 / log10(n).
 *                  Antithetic chains give ESS > n: there is no cap;
 *   EPX_DG_MCSE    sqrt(var_plus / ESS): the Monte-Carlo standard error of EPX_DG_MEAN;
 *   EPX_DG_ESS_SQ  the ESS of z = (x - MEAN)^2 by the same procedure: how well the second moments, which the precision
 *                  estimate is built from, are known.
 * Results, never faults: RHAT, ESS, MCSE and ESS_SQ are NaN when nkeep < 4, when W is not a finite number > 0 (a constant
 * coordinate, e.g. of a chain that failed at its start; any non-finite draw of the coordinate) -- MEAN and VAR are then
 * what the arithmetic gives; chains == 1 is well defined (M = 2).
 * out (host): count x P x EPX_DG_COUNT, P the context's record stride; the records behind a multi-group site's own P_k
 * coordinates are NaN.  theta == NULL: the draws, chains and nkeep of the last sampling call (error "no draws yet" before
 * one, and an error when that call did not cover every site of the range), S and chains are ignored; otherwise TEST HOOK:
 * injected draws (count, S, P) row-major, chain-major within a site, as epx_named_moments takes them (a site reads its
 * own coordinates of a record only), S a multiple of chains, 1 <= chains <= 16.  nsamp out (may be NULL): the used draws
 * n per site.  A site's centred draws of 32 coordinates are kept in LDS while they fit (about 560 draws per site);
 * longer runs read them from global memory: the same bits, slower.  No floating-point atomics: the same bits on every
 * call.  Stream-ordered, one launch, one synchronisation. */
enum epx_diag { EPX_DG_MEAN = 0, EPX_DG_VAR, EPX_DG_RHAT, EPX_DG_ESS, EPX_DG_MCSE, EPX_DG_ESS_SQ, EPX_DG_COUNT };
int epx_draw_diagnostics(epx_ctx *ctx, int k0, int count, const double *theta, int S, int chains,
                         double *out /* count * P * EPX_DG_COUNT */, int *nsamp);

/* Rank-normalised split-Rhat, bulk-ESS and tail-ESS of the same draws (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021,
 * Bayesian Analysis 16(2): what Stan reports since 2019; no counterpart in the reference's own code).  The classic Rhat
 * above is blind to chains that agree in location and differ in scale, and its ESS needs finite variances; these do not.
 * The definition, stated once; the kernel k_rank_diag (csrc/rank_diag.hip) and diagnostics.rank_diagnostics_host both
 * follow it.  Per site and sampled coordinate the used draws are those of epx_draw_diagnostics: M = 2 chains half chains of
 * length h = nkeep / 2 (an odd nkeep drops the middle draw), n = M h used draws x_i.  Rhat(s) = sqrt(var_plus / W) and
 * ESS(s) of a series s in the draws' place are EXACTLY the procedure of EPX_DG_RHAT / EPX_DG_ESS above (W, var_plus,
 * Geyer's initial positive, monotone sequence, the floor 1 / log10(n), no cap).
 *   Ranks.  r_i is the 1-based rank of x_i among the n used draws; ties are equal VALUES (==: -0.0 and +0.0 tie) and get
 *     the average rank of their run.  Normal scores z_i = Phi^-1((r_i - 3/8) / (n + 1/4)), evaluated in that form.
 *   Quantiles q_p of the n used draws: type 7 in the evaluation form of "Posterior quantiles" below; med = q_0.5.
 *   EPX_RD_RHAT_BULK  Rhat(z);
 *   EPX_RD_RHAT_FOLD  Rhat(z(zeta)), zeta_i = |x_i - med| rank-normalised the same way: sensitive to the chains' scales;
 *   EPX_RD_RHAT       max(RHAT_BULK, RHAT_FOLD);
 *   EPX_RD_ESS_BULK   ESS(z);
 *   EPX_RD_ESS_TAIL   min(ESS(I(x <= q_0.05)), ESS(I(x <= q_0.95))), the indicators 0.0 / 1.0, not rank-normalised.
 * Results, never faults: all five are NaN when nkeep < 4, when the coordinate holds any non-finite draw, and when z has no
 * finite W > 0 (a constant coordinate: every score is exactly 0); RHAT_FOLD and with it RHAT are NaN when z(zeta) has none
 * (all draws equally far from med); ESS_TAIL is NaN when either indicator's ESS is (an indicator that is constant in every
 * half chain).  chains == 1 is well defined (M = 2).
 * out (host): count x P x EPX_RD_COUNT, P the context's record stride; the records behind a multi-group site's own P_k
 * coordinates are NaN.  theta, S, chains and nsamp as epx_draw_diagnostics takes them, with the same refusals in the same
 * order.  One workgroup per (site, coordinate) keeps the coordinate's sort keys, the draws they came from and the series
 * the lag products run on in LDS, 20 bytes per used draw: at most EPX_RD_MAX_DRAWS used draws per site (the 160 KiB of a
 * compute unit less 1 KiB for the workgroup's other records); more is an error.  The work per coordinate is two sorts of n
 * keys and, per series, 8 n products for every block of 8 lags its stop rule asks for.  Every sum runs in a fixed order, no
 * atomics, nothing merged across workgroups: the same bits on every call and for a sub-range of sites.  Stream-ordered, one
 * launch, one synchronisation. */
#define EPX_RD_MAX_DRAWS 8140
enum epx_rank_diag { EPX_RD_RHAT = 0, EPX_RD_RHAT_BULK, EPX_RD_RHAT_FOLD, EPX_RD_ESS_BULK, EPX_RD_ESS_TAIL, EPX_RD_COUNT };
int epx_draw_rank_diagnostics(epx_ctx *ctx, int k0, int count, const double *theta, int S, int chains,
                              double *out /* count * P * EPX_RD_COUNT */, int *nsamp);
/* TEST HOOK, no context: the ranking stage alone, from the device functions k_rank_diag uses.  x (m x n row-major, host):
 * m series of n values, 1 <= n <= EPX_RD_MAX_DRAWS; fold != 0: |x - med| of each series is ranked instead of x.  rank_out,
 * z_out (m x n each, host): the average rank and the normal score of every value, in the values' order; NaN throughout a
 * series with a non-finite value.  Leaves the calling thread's current device as it found it. */
int epx_rank_normalize(int device, long long m, int n, const double *x, int fold, double *rank_out, double *z_out);

/* Posterior quantiles: order statistics across the draws, per site and over the pool of several sites (no counterpart in
 * the reference, whose user calls `fit.extract` and np.percentile on the host).  The definition, stated once; the kernels
 * k_site_order_stats / k_pooled_count (csrc/quantiles.inc, csrc/order_key.h) and the host restatement (quantiles.py) both
 * follow it.
 *   Order.  The draws x_0 .. x_{n-1} of one element are ordered by the key k(x): the IEEE-754 bits of x as uint64, all bits
 *     flipped if the sign bit is set, otherwise the sign bit set -- so -inf < ... < -0.0 < +0.0 < ... < +inf.  x_(r) is the
 *     value whose key has rank r ascending, 0-based; ties are the same bits, so their order does not matter.
 *   Quantile at probability p in [0, 1] (Hyndman-Fan type 7, NumPy's `linear`).  n = 1: x_(0).  Otherwise h = p (n - 1),
 *     i = min(floor(h), n - 2), g = h - i and q = x_(i) + g (x_(i+1) - x_(i)), evaluated in exactly that form in double
 *     (the library is built with -ffp-contract=off).  The HOST interpolates (quantiles.interpolate) in both routes: the
 *     device delivers order statistics, not interpolated values.
 *   Results, never faults: an element with any NaN draw has NaN at every rank and probability, that element alone; +-inf
 *     are ordered like any value and the interpolation gives what the arithmetic gives; a p outside [0, 1] or NaN is an
 *     argument error (quantiles.rank_plan).
 *
 * Per site: out[(site, element, rank)] = x_(ranks[rank]) of the element's draws at that site, count x L x n_ranks row-major,
 * L laid out as epx_named_moments lays it out (the names in the order given, at most 16, each padded to the context's
 * LARGEST site) with NaN behind a site's own elements.  ranks: ascending, distinct, in [0, draws per site), at most 32.
 * theta == NULL: the draws of the last sampling call (error "no draws yet" before one, and an error when that call did not
 * cover every site of the range), S is ignored; otherwise TEST HOOK: injected draws (count, S, P) row-major as
 * epx_named_moments takes them.  nsamp out (may be NULL): draws per site.  One workgroup per (site, element) sorts the
 * element's keys in LDS, padded to a power of two with the all-ones key (a bitonic network): at most 16384 draws per site
 * (128 KiB of keys in the 160 KiB of LDS); more is an error.  No floating-point atomics, no atomics at all: the same bits
 * on every call.  Stream-ordered, one launch, one synchronisation. */
int epx_named_order_stats(epx_ctx *ctx, int k0, int count, const int32_t *names, int n_names,
                          const int64_t *ranks, int n_ranks, const double *theta, int S,
                          double *out /* count x L x n_ranks */, int *nsamp);
/* Pooled: ONE counting pass of the selection, most significant byte first, among the draws of the sites k0..k0+count taken
 * together -- the posterior approximation of a parameter every site holds (phi, mu_a, mu_b, sigma_a, sigma_b, sigma), as
 * Master.mix_phi pools them.  The pool fits no LDS and, with several ranks, no single device; counts are integers, so they
 * add over workgroups and ranks exactly.  For every element e and target t, hist[e][t][b] = the draws of the range whose key
 * agrees with prefix[e][t] in all bits above shift + 7 and whose byte at `shift` is b; at shift = 56 every draw counts
 * (prefix may be NULL).  A NaN draw counts by its key like any other and is counted in n_nan[e] besides.  The caller runs the
 * eight passes (quantiles.select_pooled): per (element, target) it walks the cumulative counts to the byte that holds the
 * remaining rank, extends the prefix by it and reduces the rank; behind the pass at shift = 0 the prefix is the key of x_(r).
 * L = the sum of the names' lengths at the sites of the range, which have to be equal for every name (else an error).
 * n_targets: at most 32.  n out: the draws in the range, count x draws per site.  theta as above.  Counted in LDS
 * histograms with integer atomics and added to the global ones with integer atomics: the same result on every call.  The
 * workspace is the context's.  Stream-ordered, one launch, one synchronisation. */
int epx_pooled_count_pass(epx_ctx *ctx, int k0, int count, const int32_t *names, int n_names, int shift /* 56, 48, ..., 0 */,
                          const uint64_t *prefix /* L x n_targets */, int n_targets, const double *theta, int S,
                          long long *hist /* L x n_targets x 256 */, long long *n_nan /* L */, long long *n);

/* ---------------------------------------------------------------------------------------------
 * Several GPUs: sites are sharded over the ranks (one context each); the only exchange of an EP
 * iteration is the reduction of method.py:1073-1074 (Q = sum_k Qi2 + Q0 over ALL sites) and the logical
 * AND of the cavity flags (:1145).  The library runs both as RCCL all-reduces on the context's stream.
 *   rank 0:      epx_comm_unique_id(id)           -> hand the EPX_COMM_ID_BYTES bytes to every rank
 *   every rank:  epx_comm_init(ctx, id, rank, nranks)      (collective: returns when all ranks called)
 * The reference runs in one process and has no counterpart. */
#define EPX_COMM_ID_BYTES 128
enum epx_op { EPX_OP_SUM = 0, EPX_OP_MIN = 1, EPX_OP_MAX = 2 };
int epx_comm_unique_id(void *id_out);
int epx_comm_init(epx_ctx *ctx, const void *id, int rank, int nranks);
/* The same binding over a transport of the caller's (an MPI / gloo / socket all-reduce on HOST memory) for nodes
 * without RCCL peer access and for tests: `fn(buf, n, op, user)` reduces buf[n] over the ranks in place (op: enum
 * epx_op) and returns 0.  Every library collective then stages through the host: same results, one extra
 * synchronisation per collective. */
typedef int (*epx_host_allreduce_fn)(double *buf, long long n, int op, void *user);
int epx_comm_init_host(epx_ctx *ctx, int rank, int nranks, epx_host_allreduce_fn fn, void *user);
int epx_comm_destroy(epx_ctx *ctx);
/* rank and number of ranks of the context's communicator as RCCL reports them (0 of 1 without one) */
int epx_comm_size(epx_ctx *ctx, int *rank, int *nranks);
/* small host-side collectives over the communicator (staged through device memory, synchronous):
 * buf[n] reduced in place with op; in[n] of every rank gathered into out[n * nranks] in rank order.
 * Without a communicator both are the identity. */
int epx_comm_allreduce(epx_ctx *ctx, double *buf, int n, int op);
int epx_comm_allgather(epx_ctx *ctx, const double *in, int n, double *out);

/*
 * One damping trial of the update phase (method.py:1067-1143) as ONE stream-ordered batch with ONE host
 * synchronisation:  [reduce_sums: packed site sums of this rank -> all-reduce(sum) over the communicator,
 * the caller's statistics riding on the same buffer] -> Q, r for df -> Cholesky check (:1077-1080)
 * [-> S = Q^-1, m = S r with want_moments (:1211-1216)] -> cavities of all local sites against Qi + df*dQi
 * (:1138-1143) -> flags -> all-reduce(min) of the flags.
 *   reduce_sums  1 on the first trial of an iteration (or after epx_force_pd), 0 on the following ones: the
 *                proposal is affine in df, the reduced sums are kept;
 *   stat_sum[n_sum], stat_max[n_max]  in/out, only with reduce_sums, at most 8 each: summed / maximised over
 *                the ranks (the any-site-ok / all-sites-ok counts and the analytics of method.py:1043-1045);
 *   site_base    global index of the context's first site;
 *   global_pd, cav_pd  the two checks over ALL ranks; first_bad: first failing site (global index) or -1;
 *   S (d,d), m (d)  moments of the proposal (valid when both checks hold), may be NULL.
 */
int epx_update_trial(epx_ctx *ctx, double df, int reduce_sums, int site_base, double *stat_sum, int n_sum,
                     double *stat_max, int n_max, int want_moments, int *global_pd, int *cav_pd,
                     int64_t *first_bad, double *S, double *m);

/* Damping sweep (experiment/find_damp.py:146-173, the loop `for di, df in enumerate(damps)`): for every
 * dfs[i] form the proposal Q = Q0 + sum(Qi + df dQi), r likewise, factorise, S = Q^-1, m = S r, all cavities,
 * and score the proposal against a target posterior: out[i*5 + {0..4}] =
 *   global_pd (0/1), all local cavities pd (0/1), mse = mean((m - m_target)^2)      (:157),
 *   KL(N(m_target,S_target) || N(m,S))   (kl_mvn, :38-56; half_logdet_S_target = sum(log(diag(cho(S_target))))),
 *   ll = sum_s log N(x_s | m, S) over the target samples (:159-160), given by their sufficient statistics
 *        samp_mean (d), samp_scatter = sum (x_s - mean)(x_s - mean)' (d x d), n_samp  (NULL / 0: ll = NaN).
 * The criteria are NaN unless both flags are 1 (the reference leaves its pre-filled NaN there).  All trials
 * run back to back on the context's stream with one synchronisation at the end.  packed_*: as in
 * epx_damped_trial.  With several ranks the caller min-reduces column 1 (and voids rows accordingly). */
int epx_damp_sweep(epx_ctx *ctx, int ndf, const double *dfs, const double *packed_host, const double *packed_dev,
                   const double *m_target, const double *S_target, double half_logdet_S_target,
                   const double *samp_mean, const double *samp_scatter, int n_samp, double *out);

/* Scheduling hint for the next sampling calls that cover sites 0..count-1: workgroup i takes site
 * order[i] (a permutation of 0..count-1).  Workgroups are dispatched in index order, so listing the
 * sites by decreasing expected work (e.g. the leapfrogs of the previous EP iteration) shortens the
 * tail of the launch.  Results do not depend on it.  NULL / count 0 clears the hint.
 * No reference counterpart (the reference runs its sites one after the other, method.py:1005-1023). */
int epx_set_site_order(epx_ctx *ctx, const int32_t *order, int count);

/* With a site order set and the layout left to the library (epx_sampler_opts.layout 0) on a batch
 * large enough for layout 1: the first n_lead sites of the order run one workgroup per chain
 * (layout 2) on a second queue, concurrently with layout 1 for the others.  A sampling launch ends
 * with its slowest chain (max_treedepth leapfrogs in every transition); listing the sites expected
 * to hold such chains first lets them run at layout 2's shorter leapfrog.  n_lead is clamped so
 * that the lead sites occupy at most half of the CUs; 0 (default) disables.  Draws of a site are
 * those of the layout it ran in.  epx_last_split: lead sites of the last sampling call.
 * No reference counterpart. */
int epx_set_site_split(epx_ctx *ctx, int n_lead);
int epx_last_split(epx_ctx *ctx);
/* Pieced launch of the samplers that keep one workgroup per site (layouts 5, 7 and 3): with a piece queue set, a
 * sampling call over ALL sites cuts every site's run into PIECES (piece_len transitions) and runs as many workgroups as
 * the device holds at a time; a workgroup claims the site with the largest predicted remaining work (transitions left x
 * rate[site], rate = predicted leapfrogs per transition, NULL = all equal) that nobody holds, runs its next piece,
 * leaves a checkpoint at the transition boundary, puts the site back and looks for the next one until no site has
 * anything left -- longest remaining processing time first, which ends all sites at about the same time whatever they
 * really cost (a launch of one workgroup per site ends with the CU that drew two heavy sites).  Exactly the draws of
 * the plain launch.  (Environment, diagnostics only: EPX_PIECE_GRID=1 launches one workgroup per piece instead of
 * looping ones -- same draws, 1-6 % slower: the device deals a grid's workgroups to its XCDs in order.)
 * piece_len <= 0 clears.  No counterpart in the reference (scheduling only). */
int epx_set_piece_queue(epx_ctx *ctx, int piece_len, const double *rate);
/* TEST HOOK: a per-transition trace of the sampler.  With sites > 0 every sampling call (epx_tilted_batch /
 * epx_sample_batch) also records, for its first `sites` sites, ONE RECORD PER TRANSITION of every chain -- the warm-up
 * included, which the draws returned to the caller (method.py:88-104: post-warm-up only) never show:
 *   [0] step size used  [1] leapfrogs  [2] accept statistic  [3] tree depth  [4] divergent
 *   [5] step size after stepsize_adaptation::learn_stepsize / complete_adaptation (in front of the step-size search that
 *       follows a new metric)  [6] sum of the diagonal metric after var_adaptation::learn_variance  [7] log density
 *   [8 .. 8 + P) the new sample.
 * epx_get_trace copies sites x chains x iter x (8 + P) doubles.  What stands behind it in the reference is PyStan's own
 * sampler state (get_sampler_params(inc_warmup=True), /root/reference/epstan/method.py:99-102 reads stepsize__ from it);
 * tests/test_gpu_round5.py and bench.py's parity record compare it with the same trace of oracle/nuts_oracle.c. */
int epx_set_trace(epx_ctx *ctx, int sites);
/* TEST HOOK: teacher-forced transition.  Every chain of every site takes ONE transition, number t0 (0 < t0 < iter) of a
 * run with the given options, from the state in `records_in` -- per (site, chain) a checkpoint record of the pieced launch
 * (csrc/epx_pieces.h: (4 NV + 1) x 64 doubles, NV = ceil(P / 64): sample, Welford mean, Welford sum of squares, metric in
 * element order with stride NV x 64, then the 20 scalars of EPX_CK_LIST: log density, step size, dual-averaging state,
 * window counters, statistics) -- and leaves the record of boundary t0 + 1 in `records_out`: the adaptation a warm-up
 * transition performs (stepsize_adaptation::learn_stepsize, var_adaptation::learn_variance and the step-size search behind a
 * new metric) becomes comparable with oracle/nuts_oracle.c from ANY state of the oracle's run, warm-up included, without
 * the two runs having to stay together up to there.  Runs the kernels of the piece queue (layouts 5, 7, 3), one workgroup
 * per site.  With epx_set_trace the transition's trace record is available as well. */
int epx_sample_piece(epx_ctx *ctx, const int64_t *seeds, const epx_sampler_opts *opts, int t0,
                     const double *records_in, double *records_out);
int epx_get_trace(epx_ctx *ctx, double *out, long long n_out);
/* Passes over the site rows that the last sampling call's ROW TEAM made for sites k0 .. k0 + count - 1 (layout 7: the four
 * chains of a site share a pass; a pass that one chain sat out while its bookkeeping ran -- a yield -- counts, which the
 * chains' own gradient counts cannot show).  Zero for sites the other layouts sampled.  A measurement aid (bench.py's
 * pass_cycles); nothing in the reference corresponds to it. */
int epx_get_team_passes(epx_ctx *ctx, int k0, int count, double *out);
/* minus the pieces per site of the last sampling call if it ran from the piece queue, 0: one workgroup per site */
int epx_last_segments(epx_ctx *ctx);
/* Compute units of the context's device (the host-side scheduling heuristics size themselves by it). */
int epx_cu_count(epx_ctx *ctx);

/* Thread layout the last sampling call ran with (1 ... 7, see epx_sampler_opts.layout; 0 before
 * the first call).  Measurement aid: layout 3 streams the rows from HBM once per leapfrog, so its
 * roofline is the HBM one (bench.py).  No reference counterpart. */
int epx_last_layout(epx_ctx *ctx);
int epx_get_chain_stats(epx_ctx *ctx, int k0, int count, double *out);
/* TEST HOOK: uniforms/normals of the device random stream */
int epx_rng_probe(int device, uint64_t seed, int chain, uint32_t t, uint32_t kind, uint32_t a,
                  uint32_t b, double *out4);
/* TEST HOOK: the lean elementary functions of the sampler kernels (csrc/epx_device.h), one of them per call, elementwise
 * on the device: out[4 i .. 4 i + 3] = the function `kind` names at (a[i], b[i]); slots it does not fill are 0.
 *   one argument a[i], result in slot 0:  RCP rcp_d, EXP exp_d, EXP_VC exp_d_vc, LOG1P_UNIT log1p_unit_d, LOG_GE1
 *     log_ge1_d, LOG_GE1_VC log_ge1_d_vc, LOG_POS log_pos_d;
 *   LSE2_LEAN log_sum_exp2_lean(a, b), LSE2 log_sum_exp2(a, b): slot 0;  MERGE merge_weights(a, b): (lse, p_right);
 *   logit f = a[i], response y = b[i] (0.0 or 1.0):  TERMS logistic_terms: (ll, g);  SPLIT logistic_split: (lin, w, g);
 *     SPLIT2_A / SPLIT2_B logistic_split2's first / second slot and PAIR_LEAN_A / PAIR_LEAN_B logistic_pair_lean's (which
 *     takes 1/2 - y): (lin, w, g), the other slot fed a fixed finite argument.
 * An unknown kind or n < 0 is refused.  No reference counterpart. */
enum epx_math_probe_kind { EPX_MP_RCP = 0, EPX_MP_EXP, EPX_MP_EXP_VC, EPX_MP_LOG1P_UNIT, EPX_MP_LOG_GE1, EPX_MP_LOG_GE1_VC,
                           EPX_MP_LOG_POS, EPX_MP_LSE2_LEAN, EPX_MP_LSE2, EPX_MP_MERGE, EPX_MP_TERMS, EPX_MP_SPLIT,
                           EPX_MP_SPLIT2_A, EPX_MP_SPLIT2_B, EPX_MP_PAIR_LEAN_A, EPX_MP_PAIR_LEAN_B, EPX_MP_COUNT };
int epx_math_probe(int device, int kind, long long n, const double *a, const double *b, double *out);

/*
 * Stand-alone batched forms of epstan/util.py on device (no context needed):
 * util.invert_normal_params (util.py:51-125): (A,b) -> (A^-1, A^-1 b), A given
 * as SPD matrices or, with cho_form, as UPPER Cholesky factors; nb matrices of
 * order d, F-order, in place; b may be NULL; info[nb]: 0 ok, 1 not pos.def.
 */
int epx_invert_normal_params(int device, int d, int nb, double *A, double *b, int cho_form,
                             int32_t *info);
/* util.olse (util.py:128-194): shrinkage precision estimate of sample
 * covariances S (nb of order d, in place) from n draws with prior matrix P
 * (nb matrices, or NULL for the naive I/d prior). */
int epx_olse(int device, int d, int nb, double *S, int n, const double *P, int32_t *info);

#ifdef __cplusplus
}
#endif
#endif /* EPX_H */
