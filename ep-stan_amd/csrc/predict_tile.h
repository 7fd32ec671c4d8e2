// The row-tile walk of the predictive kernels, defined ONCE: k_predict, k_loo (predict.hip), k_newgroup (newgroup.inc),
// k_ppc (ppc.inc) and k_ev_terms (evidence_terms.inc) differ in where a slab's coefficient columns come from and in what
// they do with a log-likelihood, not in the walk.
//
// A wave holds a tile of 16 rows in registers as the A operand of v_mfma_f64_16x16x4_f64 (operand layout: k_moments,
// dense.hip): lane = (row lane & 15, k lane >> 4) of every step, a leading 1 that takes alpha, zeros behind 1 + D.  The
// workgroup stages a SLAB of 16 coefficient columns in LDS, coef[k][column]: k = 0 alpha, k = 1 + j beta_j, zeros behind
// 1 + D up to a multiple of 4 and behind the last column (a column is a draw, or a member of a new group's pool).  A
// slab step is: stage, barrier, product, link of the lane's four results (rows (lane >> 4) + 4 r of the tile, column
// lane & 15), the caller's action on each, barrier.  A lane keeps its own column's partial sums over the slabs; the 16
// columns of a row are added across the lanes once per pass, in the fixed order of the DPP row steps (row16_sum,
// row16_max: psis.h).  Pass 1 adds up f and the link's value and finds the largest log-likelihood term of every row;
// pass 2 walks the same slabs again for sum (f - mean)^2 and sum exp(ll - max): two passes, never sum f^2 - n mean^2,
// and a log-mean-exp that stays finite where every term underflows.  A wave owns its rows for all columns: nothing is
// merged across waves, no atomics, the same bits on every call.
//
// Every function with a barrier in it (tile_slab, wg_reduce) is called by all 256 threads of the workgroup, with
// workgroup-uniform trip counts around it; `busy` is wave-uniform.
#pragma once
#include "epx_device.h"
#include "epx_kernels.h"
#include "named_elem.h"
#include "psis.h"                  // row16_sum, row16_max

namespace epx {

typedef double v4d __attribute__((ext_vector_type(4)));

enum { PR_KMAX = (1 + EPX_PR_DMAX + 3) / 4 * 4, PR_STEPS = PR_KMAX / 4 };

#define EPX_TILE_FN __device__ __forceinline__

// Coefficient k of a slab column: alpha (k = 0) or beta_{k - 1} of group g of a site with ng groups
EPX_TILE_FN NamedElem tile_coef_elem(const PredictModel &m, int k, int g, int ng) {
    return k == 0 ? named_elem_of(EPX_NM_ALPHA, g, m.model, m.D, m.d, m.gauss, ng)
                  : named_elem_of(EPX_NM_BETA, (m.model == EPX_M1B_SG ? 0 : g * m.D) + k - 1, m.model, m.D, m.d, m.gauss, ng);
}

// The Gaussian family's scale of the slab's 16 columns: y ~ normal(f, sigma), sigma = exp(phi[0]); th: the record of
// column threadIdx.x (read only where `in`: nothing of a record behind the last column)
EPX_TILE_FN void tile_stage_scale(const PredictModel &m, const double *th, bool in, double *lsig, double *sig) {
    if (m.gauss && threadIdx.x < 16) {
        const double ls = in ? th[0] : 0.0;
        lsig[threadIdx.x] = ls;
        sig[threadIdx.x] = exp_d(ls);
    }
}

// f of (row (lane >> 4) + 4 r, column lane & 15), r < 4, of the wave's row tile against the staged slab
EPX_TILE_FN v4d predict_product(const double (&xa)[PR_STEPS], const double *coef, int nstep, int lane) {
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    const double *cl = coef + (lane >> 4) * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < PR_STEPS; ++i) {
        if (i < nstep) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[i], cl[i * 64], acc, 0, 0, 0);
    }
    return acc;
}

// log-likelihood term of response y at linear predictor f, and the link's value `mu` (whose mean over the columns is
// EPX_PR_MEAN): sigmoid(f) / y f - log(1 + e^f), or f / the normal density's logarithm at scale sg = exp(ls)
EPX_TILE_FN void predict_link(int gauss, double f, double y, double ls, double sg, double &mu, double &ll) {
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

// A wave's tile: rows t0 .. t0 + 15 of the `rows` rows that start at sorted position `first`
struct RowTile {
    double xa[PR_STEPS];               // A operand
    int row[4];                        // result r of this lane: its row as the caller counts them, or -1 (no such row)
    double y[4];                       // ... and its response (0 without one)
};

// perm: sorted position -> row of the caller, or NULL (the rows are in order); y_of(row): the response, asked only for
// rows there are and only with has_y
template <class Y>
EPX_TILE_FN void tile_load(RowTile &t, const double *X, int D, const int *perm, int first, int rows, int t0, bool busy,
                           bool has_y, Y y_of) {
    const int lane = threadIdx.x & 63, col = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int i = 0; i < PR_STEPS; ++i) t.xa[i] = 0.0;
    if (busy && t0 + col < rows) {
        const double *x = X + (size_t)(perm ? perm[first + t0 + col] : first + t0 + col) * D;
#pragma unroll
        for (int i = 0; i < PR_STEPS; ++i) {
            const int c = 4 * i + kq;
            if (c <= D) t.xa[i] = c == 0 ? 1.0 : x[c - 1];
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int tr = t0 + kq + 4 * r;
        t.row[r] = busy && tr < rows ? (perm ? perm[first + tr] : first + tr) : -1;
        t.y[r] = has_y && t.row[r] >= 0 ? y_of((size_t)t.row[r]) : 0.0;
    }
}

struct Slab { double *coef, *lsig, *sig; };               // LDS: KP x 16 coefficients, log sigma and sigma of 16 columns

// One slab step.  stage(): all threads fill the slab; in: the lane's column exists; link: the action wants mu and ll
// (else it gets zeros); each(r, f, mu, ll): the lane's result r; close(): all threads, in front of the closing barrier.
template <class Stage, class Each, class Close>
EPX_TILE_FN void tile_slab(const RowTile &t, const Slab &sl, int gauss, int nstep, bool busy, bool in, bool link,
                           Stage stage, Each each, Close close) {
    const int lane = threadIdx.x & 63, col = lane & 15;
    stage();
    __syncthreads();
    if (busy) {
        const v4d f = predict_product(t.xa, sl.coef, nstep, lane);
        if (in) {
            const double ls = gauss ? sl.lsig[col] : 0.0, sg = gauss ? sl.sig[col] : 1.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double mu = 0.0, ll = 0.0;
                if (link) predict_link(gauss, f[r], t.y[r], ls, sg, mu, ll);
                each(r, f[r], mu, ll);
            }
        }
    }
    close();
    __syncthreads();
}

// The two passes' sums of a lane's four results, and what closing them leaves
struct RowSums {
    double fm[4], sm[4], mx[4];        // pass 1: sum of f, of the link's value, largest ll -> their row means, the row's max
    double q[4], se[4];                // pass 2: sum (f - mean)^2, sum exp(ll - max)
};
EPX_TILE_FN void sums_begin(RowSums &s) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        s.fm[r] = s.sm[r] = s.q[r] = s.se[r] = 0.0;
        s.mx[r] = -INFINITY;
    }
}
EPX_TILE_FN void sums_add1(RowSums &s, int r, double f, double mu, double ll) {
    s.fm[r] += f;
    s.sm[r] += mu;
    s.mx[r] = fmax(s.mx[r], ll);
}
EPX_TILE_FN void sums_close1(RowSums &s, double n) {     // n: columns of the walk
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        s.fm[r] = row16_sum(s.fm[r]) / n;
        s.sm[r] = row16_sum(s.sm[r]) / n;
        s.mx[r] = row16_max(s.mx[r]);
    }
}
EPX_TILE_FN void sums_add2(RowSums &s, int r, double f, double ll, bool has_y) {
    const double c = f - s.fm[r];
    s.q[r] += c * c;
    if (has_y) s.se[r] += exp_d(ll - s.mx[r]);
}
// Closes pass 2 and writes the record of every row of the tile: out_of(r) is where result r's four numbers go
template <class Out>
EPX_TILE_FN void sums_close2(RowSums &s, const RowTile &t, double n, bool has_y, Out out_of) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        s.q[r] = row16_sum(s.q[r]);
        s.se[r] = row16_sum(s.se[r]);
        if ((threadIdx.x & 15) == 0 && t.row[r] >= 0) {
            double *o = out_of(r);
            o[EPX_PR_MEAN] = s.sm[r];
            o[EPX_PR_F_MEAN] = s.fm[r];
            o[EPX_PR_F_M2] = s.q[r];
            o[EPX_PR_LPD] = has_y ? s.mx[r] + log_pos_d(s.se[r] / n) : NAN;
        }
    }
}

// op over the workgroup of a value per thread that the 16 lanes of a row have reduced already (row16_sum, row16_max):
// the 16 rows through LDS, in a fixed order
template <class Op>
EPX_TILE_FN double wg_reduce(double v, double *scr, Op op) {
    __syncthreads();
    if ((threadIdx.x & 15) == 0) scr[threadIdx.x >> 4] = v;
    __syncthreads();
    double o = scr[0];
    for (int i = 1; i < 16; ++i) o = op(o, scr[i]);
    return o;
}

}  // namespace epx
