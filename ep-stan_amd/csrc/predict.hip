// Posterior predictive of NEW rows from the draws the sampler left in device memory: for a new row x_i in group g of a
// site, the linear predictor f_si = alpha_g(s) + x_i . beta_g(s) of every draw s of the site (alpha, beta as
// named_elem.h / site_params.named_draws form them from a draw), pushed through the model's link and averaged over the
// draws.  Per row (enum epx_pred, include/epx.h): the mean of sigmoid(f) ("b" family) or of f ("a" family), the mean of
// f, the CENTRED sum of squares of f, and the log predictive density log (1/S) sum_s exp(ll_si) of a given response.
// Only the four numbers per row leave the device; site_params.predict_host states the same in NumPy.
//
// A workgroup of four waves takes up to 64 rows of ONE (site, group), a tile of 16 rows per wave (the host sorted the
// rows and cut them: PredictWg), and walks the site's draws in slabs of 16:
//   - all 256 threads stage the slab's coefficients in LDS, coef[k][draw]: k = 0 alpha, k = 1 + j beta_j, zeros behind
//     1 + D up to a multiple of 4 and behind the last draw; the exp of the log-scales is applied once, here;
//   - every wave multiplies its 16 x KP row tile (registers; a leading 1 for alpha) by the KP x 16 block with
//     v_mfma_f64_16x16x4_f64 (operand layout: k_moments, dense.hip) and applies the link to its four results per lane.
// Pass 1 adds up f and the link's mean and finds the largest log-likelihood term of every row; pass 2 walks the same
// slabs again (from L2) for sum (f - mean)^2 and sum exp(ll - max): two passes, never sum f^2 - S mean^2, and a
// log-mean-exp that stays finite where every term underflows.  A lane keeps its own draw column's partial sums over the
// slabs; the 16 columns of a row are added across the lanes once per pass, in the fixed order of the DPP row steps.  A
// wave owns its rows for all draws: nothing is merged across waves, no atomics, the same bits on every call.
#include "epx_device.h"
#include "epx_kernels.h"
#include "named_elem.h"
#include "psis.h"                  // row16_sum, row16_max; the per-row stage of k_loo

namespace epx {

typedef double v4d __attribute__((ext_vector_type(4)));

enum { PR_KMAX = (1 + EPX_PR_DMAX + 3) / 4 * 4, PR_STEPS = PR_KMAX / 4 };

// The slab's coefficient block: thread = (draw tid & 15, coefficients tid >> 4, + 16, ...).  A site reads only its own
// coordinates of a record (named_elem_of's indices), and nothing of a record behind the last draw.
__device__ inline void predict_stage(const PredictArgs &a, const double *TH, int s0, int g, int ng, double *coef,
                                     double *lsig, double *sig) {
    const int tid = threadIdx.x, t = tid & 15, s = s0 + t;
    const double *th = TH + (size_t)s * a.P;
    for (int k = tid >> 4; k < a.KP; k += 16) {
        double v = 0.0;
        if (s < a.S && k <= a.D) {
            const NamedElem el = k == 0 ? named_elem_of(EPX_NM_ALPHA, g, a.model, a.D, a.d, a.gauss, ng)
                                        : named_elem_of(EPX_NM_BETA, (a.model == EPX_M1B_SG ? 0 : g * a.D) + k - 1,
                                                        a.model, a.D, a.d, a.gauss, ng);
            v = named_value(el, th);
        }
        coef[k * 16 + t] = v;
    }
    if (a.gauss && tid < 16) {                            // y ~ normal(f, sigma), sigma = exp(phi[0])
        const double ls = s < a.S ? th[0] : 0.0;
        lsig[tid] = ls;
        sig[tid] = exp_d(ls);
    }
}

// f of (row (lane >> 4) + 4 r, draw lane & 15), r < 4, of the wave's row tile against the staged slab
__device__ inline v4d predict_product(const double (&xa)[PR_STEPS], const double *coef, int nstep, int lane) {
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    const double *cl = coef + (lane >> 4) * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < PR_STEPS; ++i) {
        if (i < nstep) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[i], cl[i * 64], acc, 0, 0, 0);
    }
    return acc;
}

// log-likelihood term of response y at linear predictor f, and the link's value `mu` (whose mean over the draws is
// EPX_PR_MEAN): sigmoid(f) / y f - log(1 + e^f), or f / the normal density's logarithm at scale sg = exp(ls)
__device__ inline void predict_link(int gauss, double f, double y, double ls, double sg, double &mu, double &ll) {
    if (gauss) {
        const double z = (y - f) / sg;
        mu = f;
        ll = -0.91893853320467274178 - ls - 0.5 * (z * z);
    } else {
        double ll0, g0;
        logistic_terms(f, 0.0, ll0, g0);                  // -log(1 + e^f), -sigmoid(f)
        mu = -g0;
        ll = y * f + ll0;
    }
}

__global__ void __launch_bounds__(256)
k_predict(PredictArgs a) {
    __shared__ double coef[PR_KMAX * 16];
    __shared__ double lsig[16], sig[16];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const PredictWg w = a.wg[blockIdx.x];
    const int S = a.S, D = a.D, nstep = a.KP / 4;
    const int k = a.k0 + w.site, g = w.group;
    const int ng = a.site_g0 ? a.site_g0[k + 1] - a.site_g0[k] : 1;
    const double *TH = a.draws + (size_t)w.site * S * a.P;
    const int t0 = wave * EPX_PR_TILE;                    // the wave's tile: rows t0 .. t0 + 15 of the workgroup's
    const bool busy = t0 < w.rows;                        // (wave-uniform: a wave without rows only stages)
    const bool has_y = a.y != nullptr;

    // A operand: lane = (row col, k kq) of every step; column 0 of the tile is the 1 that takes alpha
    double xa[PR_STEPS];
#pragma unroll
    for (int i = 0; i < PR_STEPS; ++i) xa[i] = 0.0;
    if (busy && t0 + col < w.rows) {
        const double *x = a.X + (size_t)a.perm[w.first + t0 + col] * D;
#pragma unroll
        for (int i = 0; i < PR_STEPS; ++i) {
            const int c = 4 * i + kq;
            if (c <= D) xa[i] = c == 0 ? 1.0 : x[c - 1];
        }
    }
    // results: lane = (rows kq + 4 r, draw col)
    int orow[4];
    double yv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int tr = t0 + kq + 4 * r;
        orow[r] = busy && tr < w.rows ? a.perm[w.first + tr] : -1;
        yv[r] = has_y && orow[r] >= 0 ? a.y[orow[r]] : 0.0;
    }

    // ---- pass 1: sums of f and of the link's value, the largest log-likelihood term
    double sf[4] = {0.0, 0.0, 0.0, 0.0}, sm[4] = {0.0, 0.0, 0.0, 0.0};
    double mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int s0 = 0; s0 < S; s0 += 16) {
        predict_stage(a, TH, s0, g, ng, coef, lsig, sig);
        __syncthreads();
        if (busy) {
            const v4d f = predict_product(xa, coef, nstep, lane);
            if (s0 + col < S) {
                const double ls = a.gauss ? lsig[col] : 0.0, sg = a.gauss ? sig[col] : 1.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double mu, ll;
                    predict_link(a.gauss, f[r], yv[r], ls, sg, mu, ll);
                    sf[r] += f[r];
                    sm[r] += mu;
                    mx[r] = fmax(mx[r], ll);
                }
            }
        }
        __syncthreads();
    }
    double fm[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        fm[r] = row16_sum(sf[r]) / (double)S;
        sm[r] = row16_sum(sm[r]) / (double)S;
        mx[r] = row16_max(mx[r]);
    }

    // ---- pass 2: centred squares of f, sum exp(ll - max)
    double q[4] = {0.0, 0.0, 0.0, 0.0}, se[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s0 = 0; s0 < S; s0 += 16) {
        predict_stage(a, TH, s0, g, ng, coef, lsig, sig);
        __syncthreads();
        if (busy) {
            const v4d f = predict_product(xa, coef, nstep, lane);
            if (s0 + col < S) {
                const double ls = a.gauss ? lsig[col] : 0.0, sg = a.gauss ? sig[col] : 1.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double c = f[r] - fm[r];
                    q[r] += c * c;
                    if (has_y) {
                        double mu, ll;
                        predict_link(a.gauss, f[r], yv[r], ls, sg, mu, ll);
                        se[r] += exp_d(ll - mx[r]);
                    }
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        q[r] = row16_sum(q[r]);
        se[r] = row16_sum(se[r]);
        if (col == 0 && orow[r] >= 0) {
            double *o = a.out + (size_t)orow[r] * EPX_PR_COUNT;
            o[EPX_PR_MEAN] = sm[r];
            o[EPX_PR_F_MEAN] = fm[r];
            o[EPX_PR_F_M2] = q[r];
            o[EPX_PR_LPD] = has_y ? mx[r] + log_pos_d(se[r] / (double)S) : NAN;
        }
    }
}

#include "newgroup.inc"              // k_newgroup, k_newgroup_merge, k_newgroup_latents: a group that was not in the data

// ---------------------------------------------------------------------------------------------------------------------
// Leave-one-out cross-validation of the context's OWN rows (include/epx.h, enum epx_loo; loo.loo_host is the NumPy
// statement).  A workgroup takes work items of up to `tiles` x 16 rows of ONE (site, group), in the context's row order
// (no permutation: a site's rows are stored group by group), one after the other:
//   1. the likelihood tile.  Wave w < tiles owns rows 16 w .. 16 w + 15 of the item for ALL draws: the slabs of 16 draws
//      are staged and multiplied as in k_predict (predict_stage / predict_product / predict_link, ONE pass), and the
//      16 x S log-likelihoods go to the tile, row-major at `stride` doubles per row -- in LDS while tiles >= 1 fit behind
//      the fixed part, else in this workgroup's slab of the context's workspace (the host sizes it by the GRID, which it
//      caps: a workgroup walks its items).  stride = S rounded up to 16, odd in units of 16: the two rows that share a
//      32-lane group of a ds_read_b64 / ds_write_b64 then sit 32 banks apart, whether they read their own 16 consecutive
//      draws or one broadcast draw each.
//   2. the per-row stage.  All 256 threads, whatever `tiles`: row rr of the item is taken by the 16 lanes tid >> 4 ==
//      rr mod 16 -- LPD exactly as k_predict forms it (a lane's draws s = c, c + 16, ... in order, then row16_sum: the
//      same bits for the same ll), LL_MEAN, the centred LL_M2 in a second pass, and psis_row (psis.h).
// Both homes of the tile hold the same numbers and the per-row stage is the same code: the same bits.
__device__ inline void loo_rows(const LooArgs &a, const PredictWg &w, const double *tile, double *scr) {
    const int tid = threadIdx.x, c = tid & 15, S = a.p.S;
    double *my = scr + (size_t)(tid >> 4) * psis_scratch_doubles(a.M);
    for (int rr = tid >> 4; rr < w.rows; rr += 16) {
        const double *ll = tile + (size_t)rr * a.stride;
        double *o = a.out + (size_t)(w.first + rr - a.row0) * EPX_LO_COUNT;
        if (!psis_row_finite(ll, S, c)) {
            if (c < EPX_LO_COUNT) o[c] = NAN;
            continue;
        }
        double sl = 0.0, mx = -INFINITY;
        for (int s = c; s < S; s += 16) {
            sl += ll[s];
            mx = fmax(mx, ll[s]);
        }
        const double mean = row16_sum(sl) / (double)S;
        mx = row16_max(mx);
        double q = 0.0, se = 0.0;
        for (int s = c; s < S; s += 16) {
            const double dl = ll[s] - mean;
            q += dl * dl;
            se += exp_d(ll[s] - mx);
        }
        q = row16_sum(q);
        se = row16_sum(se);
        const PsisOut ps = psis_row(ll, S, a.M, a.mfit, my, c);
        if (c == 0) {
            o[EPX_LO_LPD] = mx + log_pos_d(se / (double)S);
            o[EPX_LO_LL_MEAN] = mean;
            o[EPX_LO_LL_M2] = q;
            o[EPX_LO_ELPD] = ps.elpd;
            o[EPX_LO_KHAT] = ps.khat;
            o[EPX_LO_WESS] = ps.wess;
        }
    }
}

__global__ void __launch_bounds__(256)
k_loo(LooArgs a) {
    extern __shared__ __attribute__((aligned(16))) double loo_lds[];
    const PredictArgs &p = a.p;
    double *coef = loo_lds, *lsig = coef + p.KP * 16, *sig = lsig + 16, *scr = sig + 16;
    double *tile_lds = scr + 16 * psis_scratch_doubles(a.M);
    double *tile_ws = a.slab ? a.slab + (size_t)blockIdx.x * 16 * a.tiles * a.stride : nullptr;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int S = p.S, D = p.D, nstep = p.KP / 4;
    const int t0 = wave * EPX_PR_TILE;

    for (int wi = blockIdx.x; wi < a.nwg; wi += gridDim.x) {
        const PredictWg w = p.wg[wi];
        const int k = p.k0 + w.site, g = w.group;
        const int ng = p.site_g0 ? p.site_g0[k + 1] - p.site_g0[k] : 1;
        const double *TH = p.draws + (size_t)w.site * S * p.P;
        const bool busy = wave < a.tiles && t0 < w.rows;  // (wave-uniform: a wave without rows only stages)

        double xa[PR_STEPS];
#pragma unroll
        for (int i = 0; i < PR_STEPS; ++i) xa[i] = 0.0;
        if (busy && t0 + col < w.rows) {
            const double *x = p.X + (size_t)(w.first + t0 + col) * D;
#pragma unroll
            for (int i = 0; i < PR_STEPS; ++i) {
                const int cc = 4 * i + kq;
                if (cc <= D) xa[i] = cc == 0 ? 1.0 : x[cc - 1];
            }
        }
        bool live[4];
        double yv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int tr = t0 + kq + 4 * r;
            live[r] = busy && tr < w.rows;
            const size_t row = (size_t)w.first + tr;
            yv[r] = !live[r] ? 0.0 : p.gauss ? a.yd[row] : (double)a.y8[row];
        }
        for (int s0 = 0; s0 < S; s0 += 16) {
            predict_stage(p, TH, s0, g, ng, coef, lsig, sig);
            __syncthreads();
            if (busy) {
                const v4d f = predict_product(xa, coef, nstep, lane);
                if (s0 + col < S) {
                    const double ls = p.gauss ? lsig[col] : 0.0, sg = p.gauss ? sig[col] : 1.0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double mu, ll;
                        predict_link(p.gauss, f[r], yv[r], ls, sg, mu, ll);
                        const size_t at = (size_t)(t0 + kq + 4 * r) * a.stride + s0 + col;
                        if (live[r]) {
                            if (tile_ws) tile_ws[at] = ll;
                            else tile_lds[at] = ll;
                        }
                    }
                }
            }
            __syncthreads();
        }
        if (tile_ws) loo_rows(a, w, tile_ws, scr);
        else loo_rows(a, w, tile_lds, scr);
        __syncthreads();                                  // the next item overwrites the tile
    }
}

// The per-row stage alone on log-likelihoods the caller gives, (n, S) row-major in global memory: 16 rows per workgroup
// step, 16 lanes per row, psis_row reading the rows where they are.  NaN in all three for a row with a non-finite entry.
__global__ void __launch_bounds__(256)
k_psis_rows(PsisRowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double psis_lds[];
    const int tid = threadIdx.x, c = tid & 15;
    double *my = psis_lds + (size_t)(tid >> 4) * psis_scratch_doubles(a.M);
    for (long long row = (long long)blockIdx.x * 16 + (tid >> 4); row < a.n; row += (long long)gridDim.x * 16) {
        const double *ll = a.ll + (size_t)row * a.S;
        double *o = a.out + (size_t)row * 3;
        if (!psis_row_finite(ll, a.S, c)) {
            if (c < 3) o[c] = NAN;
            continue;
        }
        const PsisOut ps = psis_row(ll, a.S, a.M, a.mfit, my, c);
        if (c == 0) { o[0] = ps.elpd; o[1] = ps.khat; o[2] = ps.wess; }
    }
}

}  // namespace epx
