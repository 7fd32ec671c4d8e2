// Geyer's initial positive, monotone sequence as include/epx.h (EPX_DG_ESS) states it: what ONE thread does with a block
// of LB consecutive lags' mean autocovariances.  Shared by k_draw_diag (draw_diag.hip) and k_rank_diag (rank_diag.hip):
// the effective sample size of a rank-normalised series is defined as exactly this procedure.
#pragma once
#include <hip/hip_runtime.h>

namespace epx {

// rho[j]: on entry the mean over the half chains of acov_m(t0 + j), on exit rho(t0 + j).  The block at t0 = 0 sets W and
// var_plus (`between`: var(mean_m, ddof = 1)) and ends a series without a finite W > 0: a constant one, or a non-finite
// draw.  prev, pairs, done: the sequence's state, INFINITY, 0.0, 0 in front of the first block; done = 1 ends it.
template <int LB>
__device__ inline void geyer_block(double (&rho)[LB], int t0, int h, double between, double &W, double &var_plus,
                                   double &prev, double &pairs, int &done) {
    if (t0 == 0) {
        W = rho[0] * (double)h / (double)(h - 1);
        var_plus = W * (double)(h - 1) / (double)h + between;
        if (!(W > 0.0) || !isfinite(W)) done = 1;        // constant, or a non-finite draw
    }
#pragma unroll
    for (int j = 0; j < LB; ++j) rho[j] = 1.0 - (W - rho[j]) / var_plus;
#pragma unroll
    for (int j = 0; j < LB; j += 2) {
        if (done) break;
        const int t = t0 + j;
        if (t + 1 >= h) { done = 1; break; }
        double p = (t == 0 ? 1.0 : rho[j]) + rho[j + 1];
        if (!(p > 0.0)) { done = 1; break; }
        p = p < prev ? p : prev;
        prev = p;
        pairs += p;
    }
}

// n / tau of a finished sequence, tau floored at tau_min = 1 / log10(n); no cap
__device__ inline double geyer_ess(long long n, double pairs, double tau_min) {
    const double tau = -1.0 + 2.0 * pairs;
    return (double)n / (tau > tau_min ? tau : tau_min);
}

}  // namespace epx
