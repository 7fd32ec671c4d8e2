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

namespace epx {

typedef double v4d __attribute__((ext_vector_type(4)));

enum { PR_KMAX = (1 + EPX_PR_DMAX + 3) / 4 * 4, PR_STEPS = PR_KMAX / 4 };

// all 16 lanes of a DPP row (one output row's draw columns) end with the row's sum / maximum
__device__ inline double row16_sum(double v) {
    v += dpp_d<DPP_QUAD_XOR1>(v);
    v += dpp_d<DPP_QUAD_XOR2>(v);
    v += dpp_d<DPP_ROW_HALF_MIRROR>(v);
    v += dpp_d<DPP_ROW_MIRROR>(v);
    return v;
}
__device__ inline double row16_max(double v) {
    v = fmax(v, dpp_d<DPP_QUAD_XOR1>(v));
    v = fmax(v, dpp_d<DPP_QUAD_XOR2>(v));
    v = fmax(v, dpp_d<DPP_ROW_HALF_MIRROR>(v));
    v = fmax(v, dpp_d<DPP_ROW_MIRROR>(v));
    return v;
}

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

}  // namespace epx
