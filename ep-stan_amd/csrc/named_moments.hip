// Per-site moments of the NAMED parameters of the site models (alpha, beta, sigma_a, ...) from the draws the sampler
// left in device memory: what Master.mix_pred (/root/reference/epstan/method.py:1304-1478; experiment/fit.py:408-421)
// combines over the sites.  The reference pulls every draw of every worker through `fit.extract`; here only the
// per-site (mean, centred sum of squares) records leave the device.
//
// A bandwidth kernel: one workgroup per site reads the site's (S, P) block twice (the second pass comes from L2) and
// applies the `transformed parameters` of experiment/models/m{1..5}{a,b}[_sg].stan on the fly (site_params.py states
// them in NumPy).  Two passes -- mean first, then sum (x - mean)^2 -- never sum x^2 - n mean^2.
#include "epx_device.h"
#include "epx_kernels.h"
#include "named_elem.h"

namespace epx {

// output element e of a call's row: element r of its n-th requested name (named_elem.h)
__device__ inline NamedElem named_elem(const NamedArgs &a, int e, int ng) {
    int n = 0;
    while (n + 1 < a.n_names && e >= a.off[n + 1]) ++n;
    return named_elem_of(a.name[n], e - a.off[n], a.model, a.D, a.d, a.gauss, ng);
}

// Grid: one workgroup per site, 256 threads.  thread = (element, slice of the draws): consecutive lanes take consecutive
// elements -- consecutive coordinates of a row for every name -- and slice sl takes the draws sl, sl + nsl, ...; the
// slices are merged in slice order by the element's first thread (no atomics: the same bits on every call).  Rows with
// more than 256 elements: one thread per element walks all draws.
__global__ void __launch_bounds__(256)
k_named_moments(NamedArgs a) {
    __shared__ double part[256];
    __shared__ double mean_s[256];
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x, S = a.S, P = a.P, L = a.L;
    const int k = a.k0 + b;
    const int ng = a.site_g0 ? a.site_g0[k + 1] - a.site_g0[k] : 1;
    const double *X = a.draws + (size_t)b * S * P;
    double *mean = a.mean + (size_t)b * L, *m2 = a.m2 + (size_t)b * L;
    const double inv_S = 1.0 / (double)S;
    if (L > T) {
        for (int e = tid; e < L; e += T) {
            const NamedElem el = named_elem(a, e, ng);
            double s = 0.0, q = 0.0;
            if (el.kind != NM_ZERO) {
#pragma unroll 4
                for (int t = 0; t < S; ++t) s += named_value(el, X + (size_t)t * P);
                s *= inv_S;
#pragma unroll 4
                for (int t = 0; t < S; ++t) {
                    const double c = named_value(el, X + (size_t)t * P) - s;
                    q += c * c;
                }
            }
            mean[e] = s;
            m2[e] = q;
        }
        return;
    }
    const int nsl = T / L;
    const int e = tid % L, sl = tid / L;
    const bool active = sl < nsl;
    NamedElem el = {NM_ZERO, 0, 0, 0};
    if (active) el = named_elem(a, e, ng);
    double s = 0.0;
    if (el.kind != NM_ZERO) {
#pragma unroll 4
        for (int t = sl; t < S; t += nsl) s += named_value(el, X + (size_t)t * P);
    }
    part[tid] = s;
    __syncthreads();
    if (tid < L) {
        double m = 0.0;
        for (int i = 0; i < nsl; ++i) m += part[i * L + tid];
        mean_s[tid] = m * inv_S;
    }
    __syncthreads();
    double q = 0.0;
    if (el.kind != NM_ZERO) {
        const double m = mean_s[e];
#pragma unroll 4
        for (int t = sl; t < S; t += nsl) {
            const double c = named_value(el, X + (size_t)t * P) - m;
            q += c * c;
        }
    }
    part[tid] = q;                 // (nobody reads `part` behind the barrier that followed the merge of the means)
    __syncthreads();
    if (tid < L) {
        double v = 0.0;
        for (int i = 0; i < nsl; ++i) v += part[i * L + tid];
        mean[tid] = mean_s[tid];
        m2[tid] = v;
    }
}

}  // namespace epx

// k_site_order_stats, k_pooled_count: the order statistics of the same elements (Master.mix_quantiles)
#include "quantiles.inc"
