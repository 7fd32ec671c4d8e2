// Order statistics across the draws the sampler left in device memory: what Master.mix_quantiles interpolates into the
// credible intervals of the named parameters (include/epx.h, "Posterior quantiles", states the definition; quantiles.py
// restates it in NumPy).  The reference has no counterpart: its user pulls every draw through `fit.extract` and calls
// np.percentile.
//
//   k_site_order_stats  one workgroup per (site, element): the element's S draws become keys (order_key.h) in LDS, a
//                       bitonic network over the next power of two sorts them, the asked ranks go back as doubles.
//   k_pooled_count      one pass of the selection by counting over the POOL of several sites' draws, which fits no LDS
//                       and, with several ranks, no single device: per (element, target) a 256-bin histogram of the byte
//                       at `shift` among the draws whose higher bits agree with the target's prefix.  Integer counts add
//                       exactly, over workgroups and over ranks, in any order.
// Elements are formed by named_elem_of / named_value (named_elem.h), as k_named_moments forms them.  That header has
// two includers, named_moments.hip and predict.hip (tests/test_build.py), so this file is no translation unit of its
// own: named_moments.hip includes it behind k_named_moments, and its kernels use that file's named_elem().
#include "order_key.h"

namespace epx {

// Grid: count x L workgroups of EPX_QT_THREADS threads, workgroup = (site b, element e), e fastest: neighbouring
// workgroups read neighbouring coordinates of the same records.  Dynamic LDS: npad keys.
__global__ void __launch_bounds__(EPX_QT_THREADS)
k_site_order_stats(OrderArgs a) {
    extern __shared__ unsigned long long qt_keys[];
    const int L = a.nm.L, S = a.nm.S, P = a.nm.P, N = a.npad, tid = threadIdx.x, T = blockDim.x;
    const int b = blockIdx.x / L, e = blockIdx.x % L;
    const int k = a.nm.k0 + b;
    const int ng = a.nm.site_g0 ? a.nm.site_g0[k + 1] - a.nm.site_g0[k] : 1;
    double *out = a.out + ((size_t)b * L + e) * a.n_ranks;
    const NamedElem el = named_elem(a.nm, e, ng);
    if (el.kind == NM_ZERO) {                              // behind the site's own elements (the same for every thread)
        if (tid < a.n_ranks) out[tid] = __builtin_nan("");
        return;
    }
    const double *X = a.nm.draws + (size_t)b * S * P;
    int bad = 0;
    for (int i = tid; i < N; i += T) {
        unsigned long long key = ORDER_KEY_PAD;
        if (i < S) {
            const double x = named_value(el, X + (size_t)i * P);
            bad |= x != x;
            key = order_key(x);
        }
        qt_keys[i] = key;
    }
    if (__syncthreads_or(bad)) {                           // a NaN draw: NaN at every rank of this element
        if (tid < a.n_ranks) out[tid] = __builtin_nan("");
        return;
    }
    // bitonic network: runs of length kk, alternately ascending and descending, merged at distances j = kk / 2 ... 1;
    // thread i of a step owns the pair (idx, idx + j) whose lower index has bit j clear
    for (int kk = 2; kk <= N; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N / 2; i += T) {
                const int idx = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                const unsigned long long lo = qt_keys[idx], hi = qt_keys[idx + j];
                const bool up = (idx & kk) == 0;
                if ((lo > hi) == up) { qt_keys[idx] = hi; qt_keys[idx + j] = lo; }
            }
            __syncthreads();
        }
    }
    if (tid < a.n_ranks) out[tid] = order_value(qt_keys[a.rank[tid]]);
}

// Grid: (ceil(L / tile), slabs) workgroups of EPX_QT_THREADS threads.  thread = (element of the tile, record lane),
// element fastest: consecutive lanes read consecutive coordinates of a record, record lanes walk the slab.  Counts go
// to the workgroup's LDS histograms and from there, where they are not zero, to the global ones; both with integer
// atomics, so the sums do not depend on the order.  At shift 56 every draw counts for every target: it is counted once,
// for target 0, and added to every target's histogram.
__global__ void __launch_bounds__(EPX_QT_THREADS)
k_pooled_count(CountArgs a) {
    extern __shared__ unsigned long long qt_smem[];
    const int L = a.nm.L, P = a.nm.P, nt = a.n_targets, E = a.tile, tid = threadIdx.x, T = blockDim.x;
    unsigned long long *pfx = qt_smem;                                         // E x nt
    unsigned int *h = reinterpret_cast<unsigned int *>(qt_smem + E * nt);      // E x nt x 256
    unsigned int *nan_s = h + E * nt * 256;                                    // E
    const int e0 = blockIdx.x * E;
    const bool top = a.shift >= 56;
    for (int i = tid; i < E * nt * 256; i += T) h[i] = 0u;
    for (int i = tid; i < E; i += T) nan_s[i] = 0u;
    for (int i = tid; i < E * nt; i += T) {
        const int e = e0 + i / nt;
        pfx[i] = (!top && e < L) ? a.prefix[(size_t)e * nt + i % nt] : 0ull;
    }
    __syncthreads();
    const int le = tid & (E - 1), e = e0 + le;
    if (e < L) {
        const NamedElem el = named_elem(a.nm, e, a.ng);
        const long long r0 = (long long)blockIdx.y * a.slab_rows;
        const long long r1 = r0 + a.slab_rows < a.n ? r0 + a.slab_rows : a.n;
        if (el.kind != NM_ZERO) {
            for (long long r = r0 + tid / E; r < r1; r += T / E) {
                const double x = named_value(el, a.nm.draws + (size_t)r * P);
                if (x != x) atomicAdd(&nan_s[le], 1u);
                const unsigned long long key = order_key(x);
                if (top) {
                    atomicAdd(&h[(le * nt) * 256 + (int)(key >> 56)], 1u);
                } else {
                    const int byte = (int)((key >> a.shift) & 255ull), above = a.shift + 8;
                    for (int t = 0; t < nt; ++t)
                        if (((key ^ pfx[le * nt + t]) >> above) == 0ull) atomicAdd(&h[(le * nt + t) * 256 + byte], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < E * nt * 256; i += T) {
        const int li = i / (nt * 256), ei = e0 + li;
        if (ei >= L) continue;
        const unsigned int v = top ? h[(li * nt) * 256 + (i & 255)] : h[i];
        if (v) atomicAdd(&a.hist[(size_t)ei * nt * 256 + (i - li * nt * 256)], (unsigned long long)v);
    }
    for (int i = tid; i < E; i += T)
        if (e0 + i < L && nan_s[i]) atomicAdd(&a.n_nan[e0 + i], (unsigned long long)nan_s[i]);
}

}  // namespace epx
