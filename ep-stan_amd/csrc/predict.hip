// Posterior predictive of NEW rows from the draws the sampler left in device memory: for a new row x_i in group g of a
// site, the linear predictor f_si = alpha_g(s) + x_i . beta_g(s) of every draw s of the site (alpha, beta as
// named_elem.h / site_params.named_draws form them from a draw), pushed through the model's link and averaged over the
// draws.  Per row (enum epx_pred, include/epx.h): the mean of sigmoid(f) ("b" family) or of f ("a" family), the mean of
// f, the CENTRED sum of squares of f, and the log predictive density log (1/S) sum_s exp(ll_si) of a given response.
// Only the four numbers per row leave the device; site_params.predict_host states the same in NumPy.
//
// A workgroup of four waves takes up to 64 rows of ONE (site, group), a tile of 16 rows per wave (the host sorted the
// rows and cut them: PredictWg), and walks the site's draws in slabs of 16, twice: the row-tile walk of predict_tile.h,
// which states the tile, the slab step, the two passes' sums and the row record.  This file adds where a slab's columns
// come from: predict_stage, the site's draws.  k_newgroup (newgroup.inc), k_loo (below), k_ppc (ppc.inc), k_predict_order
// (predict_order.inc) and k_ev_terms (evidence_terms.inc) walk the same tile.
#include "predict_tile.h"
#include "evidence.h"
#include "order_key.h"               // the keys k_predict_order (predict_order.inc) sorts

namespace epx {

// The slab's coefficient block: thread = (draw tid & 15, coefficients tid >> 4, + 16, ...).  A site reads only its own
// coordinates of a record (named_elem_of's indices), and nothing of a record behind the last draw.
__device__ inline void predict_stage(const PredictArgs &a, const double *TH, int s0, int g, int ng, const Slab &sl) {
    const int tid = threadIdx.x, t = tid & 15, s = s0 + t;
    const double *th = TH + (size_t)s * a.m.P;
    for (int k = tid >> 4; k < a.m.KP; k += 16) {
        double v = 0.0;
        if (s < a.S && k <= a.m.D) v = named_value(tile_coef_elem(a.m, k, g, ng), th);
        sl.coef[k * 16 + t] = v;
    }
    tile_stage_scale(a.m, th, s < a.S, sl.lsig, sl.sig);
}

__global__ void __launch_bounds__(256)
k_predict(PredictArgs a) {
    __shared__ double coef[PR_KMAX * 16];
    __shared__ double lsig[16], sig[16];
    const int tid = threadIdx.x, wave = tid >> 6, col = tid & 15;
    const PredictWg w = a.wg[blockIdx.x];
    const int S = a.S, gauss = a.m.gauss, nstep = a.m.KP / 4;
    const int k = a.k0 + w.site, g = w.group;
    const int ng = a.site_g0 ? a.site_g0[k + 1] - a.site_g0[k] : 1;
    const double *TH = a.draws + (size_t)w.site * S * a.m.P;
    const int t0 = wave * EPX_PR_TILE;                    // the wave's tile: rows t0 .. t0 + 15 of the workgroup's
    const bool busy = t0 < w.rows;                        // (wave-uniform: a wave without rows only stages)
    const bool has_y = a.y != nullptr;
    const Slab sl{coef, lsig, sig};
    const auto stage = [&](int s0) { predict_stage(a, TH, s0, g, ng, sl); };

    RowTile t;
    tile_load(t, a.X, a.m.D, a.perm, w.first, w.rows, t0, busy, has_y, [&](size_t row) { return a.y[row]; });
    RowSums sums;
    sums_begin(sums);
    for (int s0 = 0; s0 < S; s0 += 16)
        tile_slab(t, sl, gauss, nstep, busy, s0 + col < S, true, [&] { stage(s0); },
                  [&](int r, double f, double mu, double ll) { sums_add1(sums, r, f, mu, ll); }, [] {});
    sums_close1(sums, (double)S);
    for (int s0 = 0; s0 < S; s0 += 16)
        tile_slab(t, sl, gauss, nstep, busy, s0 + col < S, has_y, [&] { stage(s0); },
                  [&](int r, double f, double mu, double ll) { sums_add2(sums, r, f, ll, has_y); }, [] {});
    sums_close2(sums, t, (double)S, has_y, [&](int r) { return a.out + (size_t)t.row[r] * EPX_PR_COUNT; });
}

#include "newgroup.inc"              // k_newgroup, k_newgroup_merge, k_newgroup_latents: a group that was not in the data

// ---------------------------------------------------------------------------------------------------------------------
// Leave-one-out cross-validation of the context's OWN rows (include/epx.h, enum epx_loo; loo.loo_host is the NumPy
// statement).  A workgroup takes work items of up to `tiles` x 16 rows of ONE (site, group), in the context's row order
// (no permutation: a site's rows are stored group by group), one after the other:
//   1. the likelihood tile.  Wave w < tiles owns rows 16 w .. 16 w + 15 of the item for ALL draws: ONE pass of the
//      row-tile walk over k_predict's slabs (predict_tile.h, predict_stage), and the 16 x S log-likelihoods go to the
//      tile, row-major at `stride` doubles per row -- in LDS while tiles >= 1 fit behind the fixed part, else in this
//      workgroup's slab of the context's workspace (the host sizes it by the GRID, which it caps: a workgroup walks its
//      items).  stride = S rounded up to 16, odd in units of 16: the two rows that share a 32-lane group of a
//      ds_read_b64 / ds_write_b64 then sit 32 banks apart, whether they read their own 16 consecutive draws or one
//      broadcast draw each.
//   2. the per-row stage.  All 256 threads, whatever `tiles`: row rr of the item is taken by the 16 lanes tid >> 4 ==
//      rr mod 16 -- LPD with the bits of k_predict's EPX_PR_LPD (the ll are those of the same walk; a lane adds its
//      draws s = c, c + 16, ... in order, then row16_sum, as the walk's two passes do: tests/test_gpu_loo.py compares
//      the bytes), LL_MEAN, the centred LL_M2 in a second pass, and psis_row (psis.h).
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
    const Slab sl{loo_lds, loo_lds + p.m.KP * 16, loo_lds + p.m.KP * 16 + 16};
    double *scr = sl.sig + 16, *tile_lds = scr + 16 * psis_scratch_doubles(a.M);
    double *tile_ws = a.slab ? a.slab + (size_t)blockIdx.x * 16 * a.tiles * a.stride : nullptr;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int S = p.S, gauss = p.m.gauss, nstep = p.m.KP / 4;
    const int t0 = wave * EPX_PR_TILE;

    for (int wi = blockIdx.x; wi < a.nwg; wi += gridDim.x) {
        const PredictWg w = p.wg[wi];
        const int k = p.k0 + w.site, g = w.group;
        const int ng = p.site_g0 ? p.site_g0[k + 1] - p.site_g0[k] : 1;
        const double *TH = p.draws + (size_t)w.site * S * p.m.P;
        const bool busy = wave < a.tiles && t0 < w.rows;  // (wave-uniform: a wave without rows only stages)

        RowTile t;
        tile_load(t, p.X, p.m.D, nullptr, w.first, w.rows, t0, busy, true,
                  [&](size_t row) { return gauss ? a.yd[row] : (double)a.y8[row]; });
        for (int s0 = 0; s0 < S; s0 += 16)
            tile_slab(t, sl, gauss, nstep, busy, s0 + col < S, true, [&] { predict_stage(p, TH, s0, g, ng, sl); },
                      [&](int r, double f, double mu, double ll) {
                          const size_t at = (size_t)(t0 + kq + 4 * r) * a.stride + s0 + col;
                          if (t.row[r] >= 0) {
                              if (tile_ws) tile_ws[at] = ll;
                              else tile_lds[at] = ll;
                          }
                      }, [] {});
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

#include "ppc.inc"                   // k_ppc, k_ppc_sites: posterior predictive checks, rows added up per draw
#include "predict_order.inc"         // k_predict_order: order statistics across draws of new rows' f or replicated response
#include "evidence_terms.inc"        // k_ev_terms: the terms of the bridge-sampling evidence estimate (evidence.hip)

}  // namespace epx
