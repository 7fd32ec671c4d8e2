// Rank-normalised split-Rhat, bulk-ESS and tail-ESS (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021) from the draws
// the sampler left in device memory; only five numbers per coordinate leave the device (enum epx_rank_diag, include/epx.h,
// where the definition is stated once; diagnostics.rank_diagnostics_host states the same in NumPy).
//
// A workgroup of 256 threads owns ONE (site, coordinate).  Dynamic LDS, 20 bytes per used draw (rank_lds_bytes):
//   key[n]  the draws' order keys (order_key.h), sorted;   idx[n]  the draw a sorted key came from;
//   s[n]    the series in draw order, [half chain][draw], that the lag products run on.
//   1. the n = M h used draws become (key, index) pairs; a non-finite draw ends the coordinate with NaN;
//   2. a bitonic network sorts the pairs by key.  Every comparator puts the smaller key at the lower position, and the
//      positions n .. 2^k - 1 are all-ones keys that are never stored: no comparator would move them;
//   3. med, q05, q95 are read from the sorted keys (type 7);
//   4. a thread finds the ends of its key's tie run by binary search (a constant coordinate is one run of n), the average
//      rank goes through normcdfinv and the score is scattered to s[index]: draw order again;
//   5. Geyer's sequence on four series in turn: z, the indicators x <= q05 and x <= q95 (formed from the sorted keys, which
//      are still there), and -- after the keys became those of |x - med| and were sorted a second time -- the folded z.
// A series (rd_series): the half chains' means (a wave per half chain), centring in place, then lags in blocks of 8.  In a
// block thread t takes the elements t, t + 256, ... of s and their products with the eight lagged neighbours: the 32
// lanes of a half wave read 32 consecutive doubles, all 64 banks once, for s[f] and for every s[f + lag].  The eight sums
// go through a wave butterfly (the same bits in every lane) and the four waves' results through LDS, added in wave order
// by thread 0, which applies the stop rule (geyer.h); the workgroup goes on while that series wants lags: each of the
// four stops at its own rule.  Two barriers per block.  Every sum runs in a fixed order, nothing is merged across
// workgroups, no atomics: the same bits on every call and for any sub-range of sites.
#include "epx_kernels.h"
#include "geyer.h"
#include "order_key.h"

namespace epx {

enum { RD_T = EPX_RD_THREADS, RD_LB = EPX_RD_LAGS, RD_W = EPX_RD_THREADS / 64 };

struct RankLds {
    uint64_t *key;
    double *s;
    uint32_t *idx;
};
__device__ inline RankLds rank_lds(void *base, int n) {
    RankLds l;
    l.key = reinterpret_cast<uint64_t *>(base);
    l.s = reinterpret_cast<double *>(l.key + n);
    l.idx = reinterpret_cast<uint32_t *>(l.s + n);
    return l;
}

// the sum over the wave's 64 lanes, in every lane: a butterfly, so every lane adds the same pairs
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// Sorts (key, idx) ascending by key, any n >= 1.  Merges of runs of length kk: the first step compares position r of a
// block with its mirror kk - 1 - r, the following ones at distances kk / 4 ... 1.  A comparator whose upper position is
// >= n is skipped: the key there would be the largest.  Ends with a barrier.
__device__ inline void rd_sort(uint64_t *key, uint32_t *idx, int n) {
    const int tid = threadIdx.x;
    int N = 1;
    while (N < n) N <<= 1;
    for (int kk = 2; kk <= N; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N / 2; i += RD_T) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                const int hi = j == kk >> 1 ? (lo | (kk - 1)) - (i & (j - 1)) : lo + j;
                if (hi < n) {
                    const uint64_t a = key[lo], b = key[hi];
                    if (a > b) {
                        const uint32_t ia = idx[lo], ib = idx[hi];
                        key[lo] = b; key[hi] = a;
                        idx[lo] = ib; idx[hi] = ia;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// type-7 quantile of the sorted keys in the form include/epx.h prescribes
__device__ inline double rd_quantile(const uint64_t *key, int n, double p) {
    if (n == 1) return order_value(key[0]);
    const double hh = p * (double)(n - 1);
    int i = (int)floor(hh);
    if (i > n - 2) i = n - 2;
    const double g = hh - (double)i, x0 = order_value(key[i]), x1 = order_value(key[i + 1]);
    return x0 + g * (x1 - x0);
}

// The average 1-based rank of the value at sorted position j.  Its tie run is the positions of equal VALUES: -0.0 and
// +0.0 have different keys and tie.  Both ends by binary search in [0, j] and [j, n - 1].
__device__ inline double rd_avg_rank(const uint64_t *key, int n, int j) {
    const uint64_t kj = key[j];
    const bool zero = order_value(kj) == 0.0;
    const uint64_t klo = zero ? order_key(-0.0) : kj, khi = zero ? order_key(0.0) : kj;
    int a = 0, b = j;                                      // the first position whose key is >= klo
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (key[mid] < klo) a = mid + 1; else b = mid;
    }
    const int first = a;
    a = j; b = n - 1;                                      // the last position whose key is <= khi
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (key[mid] > khi) b = mid - 1; else a = mid;
    }
    return 0.5 * (double)(first + a) + 1.0;
}

// (Kept out of line: inlined into a loop, normcdfinv's coefficients are hoisted into some 250 registers and the kernels
// drop to one workgroup per compute unit; as a call k_rank_diag needs 166 and three fit.)
__device__ __noinline__ double rd_score(double rank, int n) {
    return normcdfinv((rank - 0.375) / ((double)n + 0.25));
}

// s[draw] = the normal score of every sorted key's average rank.  Ends with a barrier.
__device__ inline void rd_scatter_scores(const RankLds &l, int n) {
    for (int j = threadIdx.x; j < n; j += RD_T) l.s[l.idx[j]] = rd_score(rd_avg_rank(l.key, n, j), n);
    __syncthreads();
}

// The keys become those of |x - med|, each with its draw index as before, and are sorted again.  med: the same in every
// thread, read in front of the caller's last barrier.
__device__ inline void rd_fold(const RankLds &l, int n, double med) {
    for (int j = threadIdx.x; j < n; j += RD_T) l.key[j] = order_key(fabs(order_value(l.key[j]) - med));
    __syncthreads();
    rd_sort(l.key, l.idx, n);
}

struct RdSeries {
    double W, var_plus, ess;                               // ess: NaN unless W is finite and > 0
};

// R-hat's ingredients and the ESS of the series s (M half chains of h >= 2 values, [half chain][value]), which is centred
// in place.  hm (M), part (RD_W x RD_LB), res (3): LDS.  Every thread of the workgroup calls this and gets the result.
__device__ inline RdSeries rd_series(double *s, int M, int h, double tau_min, double *hm, double *part, double *res) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = M * h;
    for (int m = wave; m < M; m += RD_W) {
        double t = 0.0;
        for (int i = lane; i < h; i += 64) t += s[m * h + i];
        t = wave_sum(t);
        if (lane == 0) hm[m] = t / (double)h;
    }
    __syncthreads();
    for (int f = tid; f < n; f += RD_T) s[f] -= hm[f / h];
    double W = NAN, var_plus = NAN, between = 0.0, prev = INFINITY, pairs = 0.0;
    int done = 0;
    if (tid == 0) {
        double t = 0.0;
        for (int m = 0; m < M; ++m) t += hm[m];
        const double mean = t / (double)M;
        for (int m = 0; m < M; ++m) {
            const double dm = hm[m] - mean;
            between += dm * dm;
        }
        between /= (double)(M - 1);
    }
    __syncthreads();
    for (int t0 = 0;; t0 += RD_LB) {
        double acc[RD_LB];
#pragma unroll
        for (int j = 0; j < RD_LB; ++j) acc[j] = 0.0;
        for (int f = tid; f < n; f += RD_T) {
            const int left = h - f % h - t0;               // lag t0 + j stays inside the half chain while j < left
            const double v = s[f];
#pragma unroll
            for (int j = 0; j < RD_LB; ++j)
                if (j < left) acc[j] += v * s[f + t0 + j];
        }
#pragma unroll
        for (int j = 0; j < RD_LB; ++j) acc[j] = wave_sum(acc[j]);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < RD_LB; ++j) part[wave * RD_LB + j] = acc[j];
        }
        __syncthreads();
        if (tid == 0) {
            double rho[RD_LB];
#pragma unroll
            for (int j = 0; j < RD_LB; ++j) {
                double t = 0.0;
                for (int w = 0; w < RD_W; ++w) t += part[w * RD_LB + j];
                rho[j] = t / ((double)h * (double)M);      // mean over the half chains of acov_m(t0 + j)
            }
            geyer_block(rho, t0, h, between, W, var_plus, prev, pairs, done);
        }
        if (!__syncthreads_or(tid == 0 && !done)) break;
    }
    if (tid == 0) {
        res[0] = W;
        res[1] = var_plus;
        res[2] = W > 0.0 && isfinite(W) ? geyer_ess((long long)n, pairs, tau_min) : NAN;
    }
    __syncthreads();
    const RdSeries r = {res[0], res[1], res[2]};
    return r;
}

// Grid: count x P workgroups of 256 threads, workgroup = (site b, coordinate e), e fastest: neighbouring workgroups read
// neighbouring coordinates of the same records.  Dynamic LDS: rank_lds_bytes(n).
__global__ void __launch_bounds__(EPX_RD_THREADS)
k_rank_diag(RankDiagArgs a) {
    extern __shared__ __align__(16) unsigned char rd_lds[];
    __shared__ double hm[2 * EPX_DG_MAX_CHAINS], part[RD_W * RD_LB], res[3];
    const int tid = threadIdx.x, P = a.P;
    const int b = blockIdx.x / P, e = blockIdx.x % P, k = a.k0 + b;
    const int Pk = a.site_g0 ? a.d + (a.site_g0[k + 1] - a.site_g0[k]) * a.pg : P;       // this site's coordinates
    const int nkeep = a.nkeep, h = nkeep / 2, M = 2 * a.chains, n = M * h;
    double *o = a.out + ((size_t)b * P + e) * EPX_RD_COUNT;
    const RankLds l = rank_lds(rd_lds, n);
    int bad = e >= Pk || h < 2;                            // (the same in every thread)
    if (!bad) {
        const double *X = a.draws + (size_t)b * a.chains * nkeep * P + e;
        for (int f = tid; f < n; f += RD_T) {
            const int m = f / h, i = f - m * h;            // m = 2 chain + half, the second half ends with the chain's last draw
            const double x = X[((size_t)(m >> 1) * nkeep + ((m & 1) ? nkeep - h : 0) + i) * P];
            bad |= !isfinite(x);
            l.key[f] = order_key(x);
            l.idx[f] = (uint32_t)f;
        }
    }
    if (__syncthreads_or(bad)) {
        if (tid < EPX_RD_COUNT) o[tid] = NAN;
        return;
    }
    rd_sort(l.key, l.idx, n);
    const double med = rd_quantile(l.key, n, 0.5), q05 = rd_quantile(l.key, n, 0.05), q95 = rd_quantile(l.key, n, 0.95);
    rd_scatter_scores(l, n);
    const RdSeries bulk = rd_series(l.s, M, h, a.tau_min, hm, part, res);
    if (!(bulk.ess == bulk.ess)) {                         // the scores have no finite W > 0: a constant coordinate
        if (tid < EPX_RD_COUNT) o[tid] = NAN;
        return;
    }
    double tail = INFINITY;
    for (int side = 0; side < 2; ++side) {
        const double q = side ? q95 : q05;
        for (int j = tid; j < n; j += RD_T) l.s[l.idx[j]] = order_value(l.key[j]) <= q ? 1.0 : 0.0;
        __syncthreads();
        const RdSeries ind = rd_series(l.s, M, h, a.tau_min, hm, part, res);
        tail = ind.ess == ind.ess && tail == tail ? fmin(tail, ind.ess) : NAN;
    }
    rd_fold(l, n, med);
    rd_scatter_scores(l, n);
    const RdSeries fold = rd_series(l.s, M, h, a.tau_min, hm, part, res);
    if (tid == 0) {
        const double rb = sqrt(bulk.var_plus / bulk.W), rf = fold.ess == fold.ess ? sqrt(fold.var_plus / fold.W) : NAN;
        o[EPX_RD_RHAT] = rf == rf ? fmax(rb, rf) : NAN;
        o[EPX_RD_RHAT_BULK] = rb;
        o[EPX_RD_RHAT_FOLD] = rf;
        o[EPX_RD_ESS_BULK] = bulk.ess;
        o[EPX_RD_ESS_TAIL] = tail;
    }
}

// TEST HOOK (epx_rank_normalize): steps 2 to 4 above, the same device functions, on series the caller gives; one
// workgroup per series; the average ranks and the scores go back in the order of the values.  A series with a non-finite
// value has NaN throughout.
__global__ void __launch_bounds__(EPX_RD_THREADS)
k_rank_normalize(RankNormArgs a) {
    extern __shared__ __align__(16) unsigned char rd_lds[];
    const int tid = threadIdx.x, n = a.n;
    const size_t at = (size_t)blockIdx.x * n;
    const RankLds l = rank_lds(rd_lds, n);
    int bad = 0;
    for (int f = tid; f < n; f += RD_T) {
        const double x = a.x[at + f];
        bad |= !isfinite(x);
        l.key[f] = order_key(x);
        l.idx[f] = (uint32_t)f;
    }
    if (__syncthreads_or(bad)) {
        for (int f = tid; f < n; f += RD_T) a.rank[at + f] = a.z[at + f] = NAN;
        return;
    }
    rd_sort(l.key, l.idx, n);
    if (a.fold) {
        const double med = rd_quantile(l.key, n, 0.5);
        __syncthreads();
        rd_fold(l, n, med);
    }
    for (int j = tid; j < n; j += RD_T) {
        const double r = rd_avg_rank(l.key, n, j);
        a.rank[at + l.idx[j]] = r;
        a.z[at + l.idx[j]] = rd_score(r, n);
    }
}

}  // namespace epx
