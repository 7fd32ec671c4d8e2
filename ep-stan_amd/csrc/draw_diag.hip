// Per-coordinate sampler diagnostics from the draws the sampler left in device memory: for every sampled coordinate of a
// site the mean, the variance estimate var_plus, split-Rhat, the effective sample size of the mean (ESS) and of the
// second moment (ESS_SQ, the same procedure on z = (x - MEAN)^2) and the Monte-Carlo standard error of the mean.  Only
// the six numbers per coordinate leave the device (enum epx_diag, include/epx.h, where the definition is stated once;
// diagnostics.diagnostics_host states the same in NumPy).
//
// A workgroup of 256 threads owns ONE site and a tile of DG_TW = 32 consecutive coordinates; thread = (coordinate
// tid & 31, slot tid >> 5).  A draw record is P contiguous doubles, so the 32 lanes of a slot read 256 contiguous bytes
// of a record, and in LDS they read 32 consecutive doubles of a tile row: all 64 banks once per half wave
// (ds_read_b64 is served in two groups of 32 lanes), no conflict for any pair of rows.  A slot takes the half chains
// slot, slot + 8, ... of its coordinate.  Per phase (x, then z):
//   1. every half chain's mean, one thread per (half chain, coordinate), the draws added in their order (k_site_stats);
//   2. the centred tile dev = value - mean_m goes to LDS, [half chain][draw][coordinate], when the site's M h draws of
//      32 coordinates fit beside the other records (DiagArgs.in_lds); otherwise every product forms its two centred
//      values from global memory again: the same arithmetic, the same bits, no limit on nkeep, slower;
//   3. lags in blocks of DG_LB = 8 (four pairs of Geyer's sequence): a thread adds up the lagged products of its half
//      chains, the coordinate's first thread adds the eight slots' partial sums in slot order and applies the stop
//      rule to the block's pairs; the workgroup goes on while any coordinate of the tile still wants lags.  A finished
//      coordinate's threads compute nothing more but still meet every barrier.
// The work is proportional to the lags the slowest coordinate of the tile needs, not to h^2.  Every sum runs in a fixed
// order, nothing is merged across workgroups, no atomics: the same bits on every call.  The z phase stages its tile in
// the same LDS; its draws come from L2.
#include "epx_kernels.h"
#include "geyer.h"

namespace epx {

enum { DG_TW = EPX_DG_TILE, DG_NS = EPX_DG_SLOTS, DG_LB = EPX_DG_LAGS };

// What the coordinate's first thread keeps of a phase.
struct DiagPhase {
    double mean, var_plus, W, ess;     // ess: NaN unless W is finite and > 0
};

// the draw's value in a phase: x, or z = (x - centre)^2
template <bool SQ>
__device__ inline double diag_value(double x, double centre) {
    if (!SQ) return x;
    const double c = x - centre;
    return c * c;
}

// X: the site's draws at this thread's coordinate (read only where `active`); hm (M x 32), tile (M h x 32, IN_LDS only),
// part (8 x 8 x 32): LDS.  Every thread of the workgroup calls this; the result is valid in the threads of slot 0.
template <bool IN_LDS, bool SQ>
__device__ inline DiagPhase diag_phase(const DiagArgs &a, const double *X, bool active, double centre, double *hm,
                                       double *tile, double *part, int *done_s) {
    const int tid = threadIdx.x, c = tid & (DG_TW - 1), slot = tid / DG_TW;
    const int nkeep = a.nkeep, h = nkeep / 2, M = 2 * a.chains;
    const size_t P = a.P;
    // 1. means of the half chains: m = 2 chain + half, the second half ends with the chain's last draw
    for (int m = slot; m < M; m += DG_NS) {
        double s = 0.0;
        if (active) {
            const double *b = X + ((size_t)(m >> 1) * nkeep + ((m & 1) ? nkeep - h : 0)) * P;
            for (int i = 0; i < h; ++i) s += diag_value<SQ>(b[(size_t)i * P], centre);
        }
        hm[m * DG_TW + c] = s / (double)h;
    }
    __syncthreads();
    // 2. the centred tile
    if (IN_LDS) {
        for (int m = slot; m < M; m += DG_NS) {
            const double *b = X + ((size_t)(m >> 1) * nkeep + ((m & 1) ? nkeep - h : 0)) * P;
            const double mu = hm[m * DG_TW + c];
            double *t = tile + (size_t)m * h * DG_TW + c;
            for (int i = 0; i < h; ++i) t[i * DG_TW] = active ? diag_value<SQ>(b[(size_t)i * P], centre) - mu : 0.0;
        }
    }
    DiagPhase r = {NAN, NAN, NAN, NAN};
    double between = 0.0, prev = INFINITY, pairs = 0.0;
    int done = 1;
    if (slot == 0) {
        double s = 0.0;
        for (int m = 0; m < M; ++m) s += hm[m * DG_TW + c];
        r.mean = s / (double)M;
        for (int m = 0; m < M; ++m) {
            const double dm = hm[m * DG_TW + c] - r.mean;
            between += dm * dm;
        }
        between /= (double)(M - 1);
        done = active ? 0 : 1;
        done_s[c] = done;
    }
    __syncthreads();
    if (h < 2) return r;                                   // (W = 0 / 0: nothing is defined; uniform over the grid)
    // 3. lag blocks
    for (int t0 = 0;; t0 += DG_LB) {
        const bool go = !done_s[c];
        if (go) {
            double acc[DG_LB];
#pragma unroll
            for (int j = 0; j < DG_LB; ++j) acc[j] = 0.0;
            const int len = h - t0;                        // lag t0 + j has len - j products
            for (int m = slot; m < M; m += DG_NS) {
                double s[DG_LB];
#pragma unroll
                for (int j = 0; j < DG_LB; ++j) s[j] = 0.0;
                if (IN_LDS) {
                    const double *t = tile + (size_t)m * h * DG_TW + c;
                    for (int i = 0; i < len; ++i) {
                        const double v = t[i * DG_TW];
#pragma unroll
                        for (int j = 0; j < DG_LB; ++j)
                            if (i + j < len) s[j] += v * t[(i + t0 + j) * DG_TW];
                    }
                } else {
                    const double *b = X + ((size_t)(m >> 1) * nkeep + ((m & 1) ? nkeep - h : 0)) * P;
                    const double mu = hm[m * DG_TW + c];
                    for (int i = 0; i < len; ++i) {
                        const double v = diag_value<SQ>(b[(size_t)i * P], centre) - mu;
#pragma unroll
                        for (int j = 0; j < DG_LB; ++j)
                            if (i + j < len) s[j] += v * (diag_value<SQ>(b[(size_t)(i + t0 + j) * P], centre) - mu);
                    }
                }
#pragma unroll
                for (int j = 0; j < DG_LB; ++j) acc[j] += s[j];
            }
#pragma unroll
            for (int j = 0; j < DG_LB; ++j) part[(slot * DG_LB + j) * DG_TW + c] = acc[j];
        }
        __syncthreads();
        if (slot == 0 && go) {
            double rho[DG_LB];
#pragma unroll
            for (int j = 0; j < DG_LB; ++j) {
                double s = 0.0;
                for (int q = 0; q < DG_NS; ++q) s += part[(q * DG_LB + j) * DG_TW + c];
                rho[j] = s / ((double)h * (double)M);      // mean over the half chains of acov_m(t0 + j)
            }
            geyer_block(rho, t0, h, between, r.W, r.var_plus, prev, pairs, done);
            done_s[c] = done;
        }
        if (!__syncthreads_or(slot == 0 && !done)) break;
    }
    if (slot == 0 && r.W > 0.0 && isfinite(r.W)) r.ess = geyer_ess((long long)M * h, pairs, a.tau_min);
    return r;
}

template <bool IN_LDS>
__device__ inline void diag_body(const DiagArgs &a, double *lds, int *done_s, double *centre_s) {
    const int tid = threadIdx.x, c = tid & (DG_TW - 1), slot = tid / DG_TW;
    const int b = blockIdx.x, k = a.k0 + b, e = blockIdx.y * DG_TW + c;
    const int Pk = a.site_g0 ? a.d + (a.site_g0[k + 1] - a.site_g0[k]) * a.pg : a.P;     // this site's coordinates
    const bool active = e < Pk;
    const int M = 2 * a.chains;
    double *part = lds, *hm = part + DG_NS * DG_LB * DG_TW, *tile = hm + (size_t)M * DG_TW;
    const double *X = a.draws + (size_t)b * a.chains * a.nkeep * a.P + e;
    const DiagPhase x = diag_phase<IN_LDS, false>(a, X, active, 0.0, hm, tile, part, done_s);
    if (slot == 0) centre_s[c] = x.mean;
    __syncthreads();
    const DiagPhase z = diag_phase<IN_LDS, true>(a, X, active, centre_s[c], hm, tile, part, done_s);
    if (slot == 0 && e < a.P) {
        double *o = a.out + ((size_t)b * a.P + e) * EPX_DG_COUNT;
        const bool ok = x.ess == x.ess;
        o[EPX_DG_MEAN] = active ? x.mean : NAN;
        o[EPX_DG_VAR] = active ? x.var_plus : NAN;
        o[EPX_DG_RHAT] = active && ok ? sqrt(x.var_plus / x.W) : NAN;
        o[EPX_DG_ESS] = active && ok ? x.ess : NAN;
        o[EPX_DG_MCSE] = active && ok ? sqrt(x.var_plus / x.ess) : NAN;
        o[EPX_DG_ESS_SQ] = active && ok ? z.ess : NAN;
    }
}

// Grid: (sites of the call, ceil(P / 32)), 256 threads; dynamic LDS: diag_lds_doubles() doubles.
__global__ void __launch_bounds__(256)
k_draw_diag(DiagArgs a) {
    extern __shared__ __align__(16) double lds[];
    __shared__ int done_s[DG_TW];
    __shared__ double centre_s[DG_TW];
    if (a.in_lds) diag_body<true>(a, lds, done_s, centre_s);
    else diag_body<false>(a, lds, done_s, centre_s);
}

}  // namespace epx
