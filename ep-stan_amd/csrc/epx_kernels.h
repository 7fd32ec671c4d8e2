// Kernel argument blocks and launch entry points shared by the .hip files and
// the C-ABI implementation (epx_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/epx.h"
#include "nuts_geometry.h"

namespace epx {

// Where a dense kernel keeps its two d x ld work matrices + 4 vectors.
struct DenseWs {
    int use_lds;        // 1: dynamic LDS, 0: global workspace
    double *global;     // per-block slots of 2*d*ld + 4*ld doubles
};

struct CavityArgs {
    int k0, d, ld;
    DenseWs ws;
    const double *Q, *r;               // global approximation (device)
    const double *Qsite, *rsite;       // site array base
    const double *dQsite, *drsite;     // optional update (proposal = site + df * update)
    size_t site_stride, rsite_stride;
    double df;
    double *cav_Om, *cav_mu;           // K x d x d, K x d
    uint8_t *flags;                    // K
};

struct MomentArgs {
    int k0, d, ld, S, prec_estim;
    DenseWs ws;
    const double *draws;               // element (site, s, i) at site*stride_site + s*stride_s + i*stride_i
    long draws_site0;
    long stride_site, stride_s, stride_i;
    const double *Q, *r;               // global approximation subtracted at method.py:457-458
    double *dQi, *dri;                 // K x d x d, K x d
    double *tilt_mean, *tilt_scatter;  // K x d, K x d x d
    uint8_t *flags;
};

// k_reweight (dense.hip; include/epx.h: epx_reweight_batch): block b takes site m.k0 + b of the context
struct ReweightArgs {
    MomentArgs m;                      // draws, sizes, the global approximation and the outputs as k_moments takes them
    const double *Om_old, *mu_old;     // the cavity the draws were sampled against: block b at + b d d, + b d (column-major)
    const double *Om_new, *mu_new;     // the cavity now, likewise
    double *rec;                       // count x EPX_RW_COUNT
    int M, mfit;                       // psis_tail_length(S), psis_fit_points(M)
    int Sp;                            // S rounded up to even
    int extra_at;                      // doubles of dynamic LDS in front of [-lr (Sp) | w (Sp) | PSIS scratch | tail draws (M ints)]
};

struct SumArgs {
    int K, d, len, nslice;
    const double *Qi, *ri, *dQi, *dri;
    double *partial;                   // nslice x len
    double *out;                       // len
};

struct GlobalArgs {
    int d, ld, want_moments;
    DenseWs ws;
    const double *packed;              // [sum Qi, sum ri, sum dQi, sum dri] or NULL (use Q,r as they are)
    const double *Q0, *r0;
    double df;
    double *Q, *r, *S, *m;
    int *flag;
    // damping sweep (find_damp.py:146-173): selection criteria of the trial against a target
    // tgt = [m_t (d), S_t (d*d), xbar (d), Sc (d*d), half_logdet_St, n_samp] ; crit = [global_pd, cav_pd, mse, kl, ll]
    const double *tgt;
    double *crit;
};

struct InvertArgs {
    int d, ld, cho_form;
    DenseWs ws;
    double *A, *b;
    int32_t *info;
};

struct OlseArgs {
    int d, ld, n;
    DenseWs ws;
    double *S;
    const double *P;
    int32_t *info;
};

struct ForceArgs {
    int d, ld;
    DenseWs ws;
    double *Qi;
    const double *dQi;
    double df, thresh, target;
    uint8_t *forced;
    double *min_eig;
};

// Named parameters of the site models from the sampled coordinates theta = [phi | eta (ng) | etb (ng x D)]
// (site_params.py restates the Stan programs; Master.mix_pred, method.py:1304-1478): elements of `name` (enum
// epx_named) at a site with ng groups, its per-site shape flattened in C order; -1: the model does not define it.
// model = the b-model id, d = dphi (the Gaussian family's leading log sigma included).
__host__ __device__ inline int named_len(int name, int model, int D, int d, int gauss, int ng) {
    const bool etb = model != EPX_M1B_SG;
    switch (name) {
    case EPX_NM_PHI: return d;
    case EPX_NM_ETA: case EPX_NM_ALPHA: return ng;
    case EPX_NM_BETA: return etb ? ng * D : D;
    case EPX_NM_SIGMA_A: return 1;
    case EPX_NM_ETB: return etb ? ng * D : -1;
    case EPX_NM_SIGMA_B: return !etb ? -1 : model == EPX_M2B_SG ? 1 : D;
    case EPX_NM_MU_A: return model >= EPX_M4B_SG ? 1 : -1;
    case EPX_NM_MU_B: return model >= EPX_M4B_SG ? D : -1;
    case EPX_NM_SIGMA: return gauss ? 1 : -1;
    default: return -1;
    }
}

enum { EPX_NM_MAX_REQ = 16 };          // names one call may ask for
struct NamedArgs {
    int model, D, d, gauss, P, S;
    int ng_max;                        // groups of the context's largest site: sizes the output row
    int k0;                            // first site (absolute: indexes site_g0)
    const int *site_g0;                // prefix sums of the groups per site, or NULL: one group everywhere
    const double *draws;               // site b of the call at draws + b * S * P: (S, P) row-major, chain-major
    int n_names, L;                    // requested names; L = off[n_names] elements per output row
    int name[EPX_NM_MAX_REQ], off[EPX_NM_MAX_REQ + 1];      // off: first element of each name's block (lengths at ng_max)
    double *mean, *m2;                 // count x L each
};
__global__ void k_named_moments(NamedArgs a);

// Order statistics across draws (quantiles.inc; include/epx.h: "Posterior quantiles").  Per site: one workgroup per (site,
// element) sorts the element's S keys (order_key.h) in LDS, padded to a power of two.
enum { EPX_QT_MAX_RANKS = 32, EPX_QT_THREADS = 256, EPX_QT_MAX_TILE = 16, EPX_QT_COUNT_LDS = 48 * 1024 };
// most draws per site whose padded keys fit the LDS: the largest power of two of 8-byte keys below lds_capacity() - 1 KiB
constexpr int order_max_draws() {
    int n = 1;
    while ((size_t)2 * n * 8 <= lds_capacity() - 1024) n *= 2;
    return n;
}
struct OrderArgs {
    NamedArgs nm;                      // model, sizes, names and draws as k_named_moments takes them (mean, m2 unused)
    int n_ranks, npad;                 // npad: S rounded up to a power of two, at least 2: keys in LDS
    int rank[EPX_QT_MAX_RANKS];        // ascending, distinct, in [0, S)
    double *out;                       // count x L x n_ranks
};
__global__ void k_site_order_stats(OrderArgs a);
// Pooled: one counting pass of the most-significant-byte-first selection over n = sites x draws records.  A workgroup
// takes `tile` elements (a power of two) and one slab of records; LDS: [prefixes | tile x n_targets x 256 counts | NaNs].
struct CountArgs {
    NamedArgs nm;                      // draws: (n, P) records; every site of the range has ng groups (equal lengths)
    int ng, shift, n_targets, tile;
    long long n, slab_rows;            // records of the range; records per slab (gridDim.y slabs, < 2^31 each)
    const unsigned long long *prefix;  // L x n_targets keys; the bits below shift + 8 are ignored
    unsigned long long *hist;          // L x n_targets x 256, zeroed by the host
    unsigned long long *n_nan;         // L, zeroed by the host
};
constexpr size_t count_lds_bytes(int tile, int n_targets) {
    return (size_t)tile * n_targets * 8 + (size_t)tile * n_targets * 256 * 4 + (size_t)tile * 4;
}
__global__ void k_pooled_count(CountArgs a);

// Pooled moments of the first d coordinates of n = sites x draws records (pooled_moments.hip; experiment/fit.py:639-646).
struct PooledArgs {
    int d, P, nt;                      // nt = ceil(d / 16) column tiles
    int want_scatter;                  // 0: the sums alone (diagonal tile pairs only, no matrix pipe)
    long long n, slab_rows;            // records; records per slab
    int nslab;
    const double *draws;               // (n, P) row-major
    const double *center;              // d, or NULL = 0
    double *part_scatter;              // nslab x pairs x 256: a pair's tile in the accumulator's element order
    double *part_sum;                  // nslab x nt x 16
    double *out_scatter, *out_sum;     // d x d column-major, d
};
__global__ void k_pooled_partial(PooledArgs a);
__global__ void k_pooled_final(PooledArgs a);

// Posterior predictive of new rows from the draws in device memory (predict.hip; include/epx.h: epx_predict).  The host
// sorts the new rows by (site, group) and cuts them into workgroups of at most 64 rows of ONE (site, group).
enum { EPX_PR_TILE = 16, EPX_PR_WG_ROWS = 64, EPX_PR_DMAX = 128 };
struct PredictWg { int site, group, first, rows; };   // site of the call; first sorted row; rows <= EPX_PR_WG_ROWS
struct PredictModel {                  // what the predictive kernels know of the context's model (predict_tile.h)
    int model, D, d, gauss, P;
    int KP;                            // 1 + D (alpha's leading 1 and the D columns) rounded up to a multiple of 4
};
struct PredictArgs {
    PredictModel m;
    int S;
    int k0;                            // first site (absolute: indexes site_g0)
    const int *site_g0;                // prefix sums of the groups per site, or NULL: one group everywhere
    const double *draws;               // site b of the call at draws + b * S * P: (S, P) row-major
    const PredictWg *wg;               // one per workgroup
    const int *perm;                   // sorted position -> row of the caller
    const double *X;                   // n x D row-major, the caller's order
    const double *y;                   // n, or NULL: no LPD
    double *out;                       // n x EPX_PR_COUNT, the caller's order
};
__global__ void k_predict(PredictArgs a);

// Posterior predictive of a group that was not in the data (newgroup.inc; include/epx.h: epx_predict_new_group).  The
// pool of N = count x S x R members is cut into chunks of whole slabs of 16 members; a work item of k_newgroup is
// (new group with rows, chunk), a workgroup walks its items.
enum { EPX_NGP_MIN_SLABS = 16, EPX_NGP_MAX_SLABS = 128, EPX_NGP_CHUNKS = 256, EPX_NGP_RMAX = 1024 };
// slabs per chunk: a function of N alone -- about EPX_NGP_CHUNKS chunks, of 16 to 128 slabs (what gll of k_newgroup holds)
constexpr int newgroup_chunk_slabs(long long N) {
    const long long nslab = (N + 15) / 16, want = (nslab + EPX_NGP_CHUNKS - 1) / EPX_NGP_CHUNKS;
    return (int)(want < EPX_NGP_MIN_SLABS ? EPX_NGP_MIN_SLABS : want > EPX_NGP_MAX_SLABS ? EPX_NGP_MAX_SLABS : want);
}
struct NewGroupArgs {
    PredictModel m;
    int E, lap;                       // latents per member: 1 (m1) or 1 + D; m5: Laplace instead of normal
    int R, chunk_slabs;
    long long N, t0;                   // pool members; pooled index of the first draw of the call
    long long nchunk, nitem;           // chunks of the pool; work items = groups with rows x nchunk
    uint64_t seed;
    int n, G;                          // rows, new groups
    const double *draws;               // (count x S, P) row-major: draw bs at draws + bs * P, phi = its first d
    const int *perm;                   // sorted (by group, stable) position -> row of the caller
    const int *gfirst;                 // G + 1: first sorted position of every group
    const int *label;                  // G: the stream's label of every group
    const int *live;                   // the groups with rows, ascending
    const double *X;                   // n x D row-major, the caller's order
    const double *y;                   // n, or NULL: no LPD, no GLPD
    double *part_rows;                 // nchunk x n (sorted positions) x EPX_PR_COUNT: the chunks' records
    double *part_grp;                  // nchunk x G: the chunks' joint terms
    double *out;                       // n x EPX_PR_COUNT, the caller's order
    double *out_group;                 // G x EPX_NG_COUNT
};
__global__ void k_newgroup(NewGroupArgs a);
__global__ void k_newgroup_merge(NewGroupArgs a);
__global__ void k_newgroup_latents(uint64_t seed, int label, long long t0, long long nt, int R, int E, int lap, double *out);

// Leave-one-out cross-validation of the context's own rows (predict.hip: k_loo; include/epx.h: epx_loo) and the per-row
// PSIS stage alone (k_psis_rows; epx_psis_rows); psis.h holds the per-row code and the sizes of its scratch.
struct LooArgs {
    PredictArgs p;                     // model, sizes, draws as k_predict takes them; X: the context's rows; wg: the work
                                       // items (first = row of the context, rows <= 16 x tiles); perm, y, out unused
    int nwg;                           // work items (a workgroup takes blockIdx.x, + gridDim.x, ...)
    const uint8_t *y8;                 // responses of the Bernoulli family ...
    const double *yd;                  // ... and of the Gaussian one
    long long row0;                    // first row of the call: row i is written at out + (i - row0) x EPX_LO_COUNT
    double *out;
    int M, mfit;                       // psis_tail_length(S), psis_fit_points(M)
    int tiles;                         // 16-row tiles (waves with rows) per work item: 4, 2 or 1
    int stride;                        // doubles per row of the log-likelihood tile
    double *slab;                      // NULL: the tile is in LDS; else gridDim.x slabs of 16 x tiles x stride doubles
};
// doubles per row of the tile: S rounded up to 16, an odd number of 16s (bank layout: predict.hip)
constexpr int loo_stride(int S) { return ((S + 15) / 16 | 1) * 16; }
__global__ void k_loo(LooArgs a);
struct PsisRowsArgs {
    long long n;
    int S, M, mfit;
    const double *ll;                  // n x S row-major
    double *out;                       // n x 3: ELPD, KHAT, WESS
};
__global__ void k_psis_rows(PsisRowsArgs a);

// Posterior predictive checks of the context's own rows (ppc.inc: k_ppc, k_ppc_sites; include/epx.h: epx_ppc).  A work
// item of k_ppc is a whole (site, group); it keeps the group's 3 x S per-draw sums in LDS.
enum { EPX_PC_WAVE_PART = 4 * 3 * 16 };                  // the four waves' partial sums of a slab: [wave][value][column]
struct PpcArgs {
    PredictArgs p;                     // model, sizes, draws as k_predict takes them; X: the context's rows; wg: the groups
                                       // of the call in order (first = row of the context, rows = ALL rows of the group);
                                       // perm, y, out unused
    int ngroups;                       // groups of the call (a workgroup takes blockIdx.x, + gridDim.x, ...)
    int count;                         // sites of the call
    const int *site_first;             // count + 1: the first group (of the call) of every site
    const uint8_t *y8;                 // responses of the Bernoulli family ...
    const double *yd;                  // ... and of the Gaussian one
    uint64_t seed;
    long long row0;                    // the stream's row of the context's row i is row0 + i
    double *per_draw;                  // ngroups x 3 x S: T_rep, D_obs, D_rep of every draw
    double *out_groups, *out_sites;    // ngroups x EPX_PC_COUNT, count x EPX_PC_COUNT
};
// doubles of dynamic LDS in front of the 3 x S per-draw sums: [coefficient slab | log sigma, sigma of the slab | wave
// partials | wg_reduce scratch | non-finite flag]
constexpr size_t ppc_fixed_doubles(int KP) { return (size_t)KP * 16 + 32 + EPX_PC_WAVE_PART + 16 + 2; }
constexpr size_t ppc_lds_bytes(int KP, int S) { return (ppc_fixed_doubles(KP) + (size_t)3 * S) * 8; }
// most draws per site whose per-draw sums fit the LDS behind the fixed part, 1 KiB left free
constexpr int ppc_max_draws(int KP) { return (int)((lds_capacity() - 1024 - ppc_fixed_doubles(KP) * 8) / 24); }
__global__ void k_ppc(PpcArgs a);
__global__ void k_ppc_sites(PpcArgs a);

// Order statistics across the draws of every NEW row's linear predictor or replicated response (predict_order.inc: k_predict_order;
// include/epx.h: epx_predict_order_stats).  A work item is up to `R` rows of one (site, group): their S x R values become
// keys (order_key.h) in LDS, row rr at rr x npad, and every row is sorted there.
struct PredOrderArgs {
    PredictArgs p;                     // model, sizes, draws, new rows, perm and work items as k_predict takes them (first =
                                       // sorted position, rows <= R); y, out unused
    int nwg;                           // work items (a workgroup takes blockIdx.x, + gridDim.x, ...)
    int what;                          // enum epx_pred_order
    int npad, lg;                      // S rounded up to a power of two, at least 2, and its logarithm
    int n_ranks;
    int rank[EPX_QT_MAX_RANKS];        // ascending, distinct, in [0, S)
    uint64_t seed;
    const uint32_t *row_id;            // n, the caller's order: the stream's index of every row; NULL: the row itself
    double *out;                       // n x n_ranks, the caller's order
};
// bytes of dynamic LDS in front of the keys, the walk's fixed part: [four times (coefficient slab | log sigma, sigma of the
// slab): a step of the walk stages 64 draws, one slab per wave | the item's 16 NaN flags]
constexpr size_t pred_order_fixed_bytes(int KP) { return (4 * ((size_t)KP * 16 + 32) + 8) * 8; }
// bytes the keys of a work item may take: what is left of the LDS, 1 KiB kept free
constexpr size_t pred_order_budget(int KP) { return lds_capacity() - 1024 - pred_order_fixed_bytes(KP); }
__global__ void k_predict_order(PredOrderArgs a);

// The site normaliser by bridge sampling (evidence.hip: k_ev_fit, k_ev_bridge; evidence_terms.inc: k_ev_terms; include/epx.h:
// epx_site_evidence).  One workgroup per site in all three kernels.
struct EvidenceArgs {
    PredictModel m;
    int S, chains, n, nh;              // draws per site; n = S / chains per chain, the first nh = n / 2 of a chain are F
    int N1;                            // |E| = chains x (n - nh) = N2
    int k0;                            // first site (absolute: indexes site_g0, the cavities)
    int pg;                            // coordinates per group: 1 (m1) or 1 + D
    const int *site_g0;                // prefix sums of the groups per site, or NULL: one group everywhere
    const double *draws;               // site b of the call at draws + b * S * P: (S, P) row-major, chain-major
    const PredictWg *wg;               // the groups of the call in order (first = row of the context, rows = ALL rows)
    const int *site_first;             // count + 1: the first group (of the call) of every site
    const double *X;                   // the context's rows
    const uint8_t *y8;                 // responses of the Bernoulli family ...
    const double *yd;                  // ... and of the Gaussian one
    const double *cav_Om, *cav_mu;     // K x d x d (column-major), K x d: the context's cavities
    uint64_t seed;
    long long site0;                   // the stream's chain of site k of the context is site0 + k
    double *fit;                       // count x evidence_fit_doubles(P): [m (P) | L packed by rows | sum log L_ii, ok]
    double *terms;                     // count x 2 N1: l1, l2
    double *prop;                      // NULL, or count x N1 x P: the proposal draws
    double *out;                       // count x EPX_EV_COUNT
    int M, mfit;                       // psis_tail_length(N1), psis_fit_points(M)
};
constexpr size_t evidence_packed(int P) { return (size_t)P * (P + 1) / 2; }
constexpr size_t evidence_fit_doubles(int P) { return (size_t)P + evidence_packed(P) + 2; }
constexpr int evidence_stride(int P) { return P | 1; }   // doubles per column of a slab's records in LDS (odd: banks)
// doubles of dynamic LDS of k_ev_terms: [L packed | m (P) | mu (P) | theta of the slab's 16 columns | their z or L^-1 (theta
// - m) | coefficient slab | log sigma, sigma | wave partials (4 x 16) | sums, base (16 each)]; k_ev_fit needs less
constexpr size_t evidence_terms_doubles(int P, int KP) {
    return evidence_packed(P) + (size_t)2 * P + (size_t)32 * evidence_stride(P) + (size_t)KP * 16 + 32 + 64 + 32;
}
// most sampled coordinates whose packed factor and workspace fit the LDS, 1 KiB left free
constexpr int evidence_max_coords(int KP) {
    int P = 1;
    while (evidence_terms_doubles(P + 1, KP) * 8 <= lds_capacity() - 1024) ++P;
    return P;
}
// doubles of dynamic LDS of k_ev_bridge: [l1 | l2 | -l2 | the iteration's terms (2 N1) | PSIS scratch | reduction scratch]
constexpr size_t evidence_bridge_doubles(int N1, int psis_scratch) { return (size_t)5 * N1 + psis_scratch + 16; }
__global__ void k_ev_fit(EvidenceArgs a);
__global__ void k_ev_terms(EvidenceArgs a);
__global__ void k_ev_bridge(EvidenceArgs a);

// Per-coordinate diagnostics of the draws in device memory (draw_diag.hip; include/epx.h: epx_draw_diagnostics).  A
// workgroup takes one site and EPX_DG_TILE coordinates; EPX_DG_SLOTS threads per coordinate share its half chains; lags
// are computed EPX_DG_LAGS at a time.
enum { EPX_DG_TILE = 32, EPX_DG_SLOTS = 8, EPX_DG_LAGS = 8, EPX_DG_MAX_CHAINS = 16 };
struct DiagArgs {
    int k0, chains, nkeep, P;          // k0: first site (absolute: indexes site_g0)
    int d, pg;
    const int *site_g0;                // multi-group sites: coordinates of site k = d + groups * pg (<= P); or NULL
    int in_lds;                        // the centred tile of a site (2 chains x (nkeep / 2) draws x 32 coordinates) is kept in LDS
    double tau_min;                    // 1 / log10(used draws): the floor of the autocorrelation time
    const double *draws;               // site b of the call at draws + b * chains * nkeep * P: chain-major records of P
    double *out;                       // count x P x EPX_DG_COUNT
};
// doubles of dynamic LDS: [slot partial sums | half-chain means | centred tile]
constexpr size_t diag_lds_doubles(int chains, int nkeep, bool in_lds) {
    return (size_t)EPX_DG_SLOTS * EPX_DG_LAGS * EPX_DG_TILE + (size_t)2 * chains * EPX_DG_TILE
        + (in_lds ? (size_t)2 * chains * (nkeep / 2) * EPX_DG_TILE : 0);
}
__global__ void k_draw_diag(DiagArgs a);

// Rank-normalised diagnostics of the draws in device memory (rank_diag.hip; include/epx.h: epx_draw_rank_diagnostics).  A
// workgroup of EPX_RD_THREADS threads takes one (site, coordinate); lags are computed EPX_RD_LAGS at a time.
enum { EPX_RD_THREADS = 256, EPX_RD_LAGS = 8 };
struct RankDiagArgs {
    int k0, chains, nkeep, P;          // as DiagArgs
    int d, pg;
    const int *site_g0;
    double tau_min;
    const double *draws;
    double *out;                       // count x P x EPX_RD_COUNT
};
// bytes of dynamic LDS for n used draws: [sort keys (8 n) | series in draw order (8 n) | draw index of a key (4 n)]
constexpr size_t rank_lds_bytes(int n) { return (size_t)n * 20; }
__global__ void k_rank_diag(RankDiagArgs a);
struct RankNormArgs {
    int n, fold;
    const double *x;                   // m x n row-major, one series per workgroup
    double *rank, *z;                  // m x n each
};
__global__ void k_rank_normalize(RankNormArgs a);

__global__ void k_cavity(CavityArgs a);
__global__ void k_moments(MomentArgs a);
__global__ void k_reweight(ReweightArgs a);
__global__ void k_site_sums_partial(SumArgs a);
__global__ void k_site_sums_final(SumArgs a);
__global__ void k_global(GlobalArgs a);
__global__ void k_axpy(double *out, const double *x, const double *dx, double df, size_t n);
__global__ void k_mix_partial(SumArgs a);
__global__ void k_sweep_flag(const int *all_flag, double *crit);
__global__ void k_all_flags(const uint8_t *flags, int k0, int count, int *out);
__global__ void k_trial_flags(const uint8_t *flags, int count, int site_base, const int *global_pd, double *out);
__global__ void k_invert(InvertArgs a);
__global__ void k_olse(OlseArgs a);
__global__ void k_force_pd(ForceArgs a);

// ------------------------------------------------------------------ sampler
enum { ST_STEPSIZE_MEAN = 0, ST_STEPSIZE_FINAL, ST_NLEAP, ST_NGRAD, ST_NDIV, ST_ACCEPT_MEAN,
       ST_DEPTH_MEAN, ST_FAIL, ST_COUNT };
enum { K_INIT = 0, K_MOM = 1, K_DIR = 2, K_TOP = 3, K_MERGE = 4, K_SSMOM = 5,
       K_NEWGROUP = 6,     // the latents of a new group (newgroup.inc): disjoint from every sampler stream
       K_PPC = 7,          // the replicated responses of a posterior predictive check (ppc.inc), likewise
       K_BRIDGE = 8,       // the proposal draws of the bridge-sampling evidence estimate (evidence.hip), likewise
       K_PRED_REP = 9 };   // the replicated responses of new rows (predict_order.inc), likewise
enum { MAX_DEPTH_CAP = 12 };
// seconds a workgroup of a pieced launch looks for a site before it reports a lost piece (epx_pieces.h); the environment
// variable of the same name overrides it at run time (NutsArgs::dyn_wait_s)
#ifndef EPX_PIECE_WAIT_S
#define EPX_PIECE_WAIT_S 60
#endif

// columns of zeros behind the last site's cavity precision (epx_api.hip allocates them): the streaming sampler's register
// ring reads up to OM_UNROLL columns past a site's Omega (nuts_stream.hip)
enum { EPX_OM_PAD_COLS = 64 };

// Default of NutsArgs::yield_cycles: cycles of s_memtime since the state wave's last job went out PLUS the estimate of the
// bookkeeping still ahead (EPX_SM_YIELD's argument) beyond which the wave lets a pass go by.  A team's pass lasts ~6 500
// cycles; a lost pass of one chain costs the team a quarter of a pass (~2 000 cycles): HISTORY.md section 3.1g (round 4)
#ifndef EPX_YIELD_DEFAULT
#define EPX_YIELD_DEFAULT 8500
#endif
struct NutsArgs {
    int gauss;                  // Gaussian-likelihood family (m*a_sg.stan): phi[0] = log sigma, real responses in yd
    const double *yd;
    int model, D, d, P;
    int k0;                       // first site of the batch
    int chains, iter, warmup, thin, nkeep, max_depth, init_mode;
    int cpb;                      // chains per block (waves per block = cpb * WPC)
    const int64_t *k_lim;         // K+1 row limits
    const double *X;              // N x D row-major
    const uint8_t *y;             // N
    const int *y32;               // N, the same responses as int32 (DMA granule of the streaming sampler)
    const double *cav_Om;         // K x d x d
    const double *cav_mu;         // K x d
    const int64_t *seeds;         // per site of the batch (index k - k0)
    const int *order;             // optional: workgroup i works on site order[i] of the batch (longest first), or NULL
    // multi-group sites (K < J; streaming layout only): groups site_g0[k]..site_g0[k+1] with the
    // absolute row limits g_lim[g]..g_lim[g+1]; NULL = one group per site.  P is then the record
    // stride (largest coordinate count over the sites).
    const int *site_g0;
    const int64_t *g_lim;
    int ngmax, ntmax;             // streaming layout: most groups / tiles of a site (LDS map)
    double *draws;                // K x chains x nkeep x P
    double *last;                 // K x chains x P (read when init_mode == PREV, always written)
    double *chain_stats;          // K x chains x ST_COUNT
    const double *eps_in;         // test hook: per (site of batch, chain) fixed step size -> no step-size search
    const double *inv_e_in;       // test hook: per (site of batch, chain) x P diagonal inverse metric
    int t_offset;                 // test hook: transition index offset of the random stream
    // opt-in `adapt = carry` (not the reference's behaviour, see include/epx.h): start from the step size the
    // chain ended the previous call with and from the site's pooled sample variances of that call as diagonal
    // metric; warm-up then adapts the step size only.  Indexed by ABSOLUTE site; NULL = adapt from scratch;
    // a non-positive step size = no history for that chain
    const double *carry_eps;      // K x chains
    const double *carry_metric;   // K x P
    unsigned long long *stamps;   // diagnostic build (-DEPX_STAMPS): per block 8 cycle sums
    int stamps_nrec;              // ... and the host's count of records per kind (the launched grid may be smaller: looping workgroups add up their pieces)
    double *dbg;                  // test hook: if set, write lp and grad of the initial point (1+P) and stop
    double *trace;                // test hook (epx_set_trace): per (site of the batch < trace_sites, chain, transition) a record of 8 + P doubles
    int trace_sites;
    double *team_passes;          // K (absolute site): passes the row team of layout 7 made over the site's rows, the ones a chain yielded
                                  // included (added up over the pieces of a queued launch); NULL = not counted
    double *stack;                // global memory of the chains of the resident layouts, indexed by (site of the batch,
                                  // chain): stack_stride doubles each -- tree stack (max_depth * (4 NV 64 + 2)) first,
                                  // then the state wave's cold store (nuts_duo.hip); one stride for every kernel of a
                                  // call, so the two kernels of a split launch can share the buffer.  Streaming layout:
                                  // nuts_stream_chain_doubles() per chain
    size_t stack_stride;
    // dynamic LDS layout (byte offsets), computed on the host
    int n_max;                    // rows reserved for X in LDS
    int off_y, off_Om, off_mu, off_xch, off_stack, lds_bytes;
    int stack_in_lds;
    int scr_doubles;              // ... its length (the P live elements, rounded up)
    int off_scr;                  // nuts_duo.hip TEAM form: per chain one vector of LDS scratch (view -> vector order)
    int stack_ps;                 // ... and the doubles one vector of such a record takes (packed: >= P)
    int stack_lds_levels;         // nuts_duo.hip, stack not (all) in LDS: the lowest levels of every chain's tree stack that are (0: none)
    int om_in_lds;
    int off_spec;                 // > 0: LDS offset of the speculative kernel's mailbox / control records (layout 2)
    int no_spec;                  // 1: keep the bookkeeping on the gradient waves (k_nuts) even when off_spec > 0
    int yield_cycles;             // row team (layout 7): a state wave whose bookkeeping of a finished subtree / transition would
                                  // end more than this many cycles after its job went out lets the team's pass go by WITHOUT a
                                  // new job of its chain (one lost pass of one chain) instead of keeping the four chains
                                  // waiting; 0 = never
    int grp;                      // 1: sites with several groups on layout 2 (k_nuts_spec<..., GRP>, nuts_gradient_groups.inc)
    int off_gl;                   // LDS offset of the site's group row limits (grp)
    // k_nuts_duo (nuts_duo.hip): row waves + state waves with LDS hand-offs
    int duo_rw;                   // row waves per chain
    int off_tail;                 // cavity precision rows 64..d-1 (row-major, stride d rounded up to even)
    int off_slot;                 // per chain: job / result slots
    int off_flag;                 // per chain: hand-off sequence numbers
    int slot_doubles;             // doubles of one chain's slots
    int off_piece;                // 16 B: (site, first transition) of the piece a persistent workgroup is running
    int *err;                     // device word: set when a hand-off spin gives up (never in a healthy run)
    // pieced launch (layout 5; epx_set_piece_queue): seg_nwg workgroups, one per piece
    int seg_nwg;
    int persist;                          // workgroups loop over claims (seg_nwg = what the device holds at a time) instead of one per piece
    double *ckpt;                 // pieced launches: per (site, chain) a record of (4 NV + 1) x 64 doubles (sample, Welford sums, metric, scalars)
    // piece queue (epx_set_piece_queue): every workgroup claims a site by largest remaining predicted work and runs
    // dyn_len transitions of it; dyn_prog[site] = 2 x transitions done + (claimed): one word, changed atomically
    int *dyn_prog, *dyn_busy;
    const double *dyn_rate;       // predicted work per transition of every site of the batch, or NULL (all equal)
    int dyn_len, dyn_count;
    const int *dyn_lens;          // per site: transitions of one of ITS pieces, or NULL (what the host gives): dyn_len for all
    int dyn_nb;                   // checkpoint records (piece boundaries) reserved per site
    int dyn_tail_div;             // the pieces behind 3/4 of a site's run are 1/dyn_tail_div of the nominal length (epx_pieces.h)
    int dyn_hook;                 // epx_sample_piece: a site is released as FINISHED behind its one transition (never claimable twice)
    int dyn_wait_s;               // seconds a workgroup looks for a site before it reports a lost piece (EPX_PIECE_WAIT_S; epx_pieces.h)
};

// launch wrapper implemented in nuts.hip; returns hipError_t as int.  The records of the LDS layouts: nuts_geometry.h
int launch_nuts(const NutsArgs &a, int count, int wpc, int dp, int nv, hipStream_t stream);
size_t nuts_lds_layout(NutsArgs &a, int wpc, int dp, int n_max);

// row-wave / state-wave variant (nuts_duo.hip): cpb chains of a site per workgroup, every chain one
// state wave + rw row waves that talk through LDS slots (no workgroup barrier in the loop)
int launch_nuts_duo(const NutsArgs &a, int count, int cpb, int rw, int dp, int nv, hipStream_t stream);
size_t nuts_duo_lds_layout(NutsArgs &a, int cpb, int rw, int dp, int n_max);
bool nuts_duo_has(int cpb, int rw, int dp, int nv);
size_t nuts_resident_chain_doubles(int nv, int max_depth);

// streaming variant (nuts_stream.hip): one workgroup per site, chains in lock step, X through
// an LDS-DMA ring; dpb in {64, 128}, nv = ceil(P/64) <= 7.  a.stack holds, per (site of the
// batch, chain), nuts_stream_chain_doubles() doubles (tree stack + cold store).
int launch_nuts_stream(const NutsArgs &a, int count, int dpb, int nv, hipStream_t stream);
size_t nuts_stream_lds_bytes(int nv, int dpb, int d, int ngmax, int ntmax, int nmax_res, int gauss);
size_t nuts_stream_chain_doubles(int nv, int max_depth);

struct RhatArgs {
    int k0, chains, nkeep, P;
    const int *site_g0;           // multi-group sites: coordinates of site k = d + groups * pg (<= P); or NULL
    int d, pg;
    const double *draws;          // K x chains x nkeep x P
    const double *chain_stats;    // K x chains x ST_COUNT
    double *site_stats;           // count x EPX_ST_COUNT (batch-relative)
};
__global__ void k_site_stats(RhatArgs a);
struct CarryArgs {
    int k0, chains, nkeep, P;
    const double *draws;          // K x chains x nkeep x P
    const double *chain_stats;    // K x chains x ST_COUNT
    double *carry_eps, *carry_metric;
};
__global__ void k_carry_update(CarryArgs a);
__global__ void k_rng_probe(uint64_t seed, int chain, uint32_t t, uint32_t kind, uint32_t a,
                            uint32_t b, double *out4);
__global__ void k_math_probe(int kind, long long n, const double *a, const double *b, double *out);   // out: n x 4

}  // namespace epx
