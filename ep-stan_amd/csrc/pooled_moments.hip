// Moments of the phi draws of MANY sites pooled, from the draws the sampler left in device memory: what the consensus
// run (/root/reference/experiment/fit.py:639-646: `samp = np.concatenate(samples)`, mean, `samp.T.dot(samp)`) forms on
// the host from every site's extracted draws.  No per-site work: no precision estimate, no factorisation, nothing of
// the site arrays is read or written.
//
// The records of the sites of a range lie back to back, (site, draw, P) row-major, and only the first d = dphi
// coordinates of a record take part -- every site has them, whatever its own number of groups -- so the pooled draws are
// ONE (n, P) matrix of which the first d columns are read: (site, slab of draws) collapses to a slab of its rows.
//
// Two kernels, the same bits on every call (no floating-point atomics):
//   k_pooled_partial  workgroup = (upper-triangle pair of 16-column tiles, slab of rows): its four waves take the slab's
//                     rows four at a time in turn, each accumulating the 16 x 16 tile of sum (x_i - c_i)(x_j - c_j) with
//                     v_mfma_f64_16x16x4_f64 (operand layout: k_moments, dense.hip); the waves' tiles are added in wave
//                     order and go to the workspace.  The diagonal pairs also add up (x_i - c_i).
//   k_pooled_final    one thread per element of the upper triangle (and of the sum) adds the slabs' partials in slab
//                     order and writes the element and its mirror image.
#include "epx_device.h"
#include "epx_kernels.h"

namespace epx {

typedef double v4d __attribute__((ext_vector_type(4)));

// pair (ti <= tj) number `tile` of the upper triangle of nt x nt tiles, row by row; diagonal pairs only: ti = tj = tile
__device__ inline void pooled_unrank(int tile, int nt, int diag_only, int &ti, int &tj) {
    if (diag_only) { ti = tj = tile; return; }
    int rem = tile;
    ti = 0;
    while (rem >= nt - ti) { rem -= nt - ti; ++ti; }
    tj = ti + rem;
}

__global__ void __launch_bounds__(256)
k_pooled_partial(PooledArgs a) {
    __shared__ double tile_s[4][256];
    __shared__ double sum_s[4][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int d = a.d, nt = a.nt;
    const size_t P = a.P;
    int ti, tj;
    pooled_unrank(blockIdx.x, nt, !a.want_scatter, ti, tj);
    const long long r0 = (long long)blockIdx.y * a.slab_rows;
    const long long r1 = r0 + a.slab_rows < a.n ? r0 + a.slab_rows : a.n;
    const int ia = ti * 16 + (lane & 15), ib = tj * 16 + (lane & 15), kq = lane >> 4;
    const bool ha = ia < d, hb = ib < d, diag = ti == tj;
    const double ca = ha && a.center ? a.center[ia] : 0.0, cb = hb && a.center ? a.center[ib] : 0.0;
    const double *X = a.draws;
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    double sa = 0.0;
    if (a.want_scatter) {
        for (long long s0 = r0 + 4 * wave; s0 < r1; s0 += 16) {
            const long long s = s0 + kq;
            double av = 0.0, bv = 0.0;
            if (s < r1) {                                       // (a column behind d is never read)
                if (ha) av = X[(size_t)s * P + ia] - ca;
                if (diag) bv = av;
                else if (hb) bv = X[(size_t)s * P + ib] - cb;
            }
            sa += av;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) tile_s[wave][r * 64 + lane] = acc[r];
    } else {
        for (long long s = r0 + 4 * wave + kq; s < r1; s += 16)
            if (ha) sa += X[(size_t)s * P + ia] - ca;
    }
    sum_s[wave][lane] = sa;
    __syncthreads();
    if (a.want_scatter) {
        // element tid = reg * 64 + lane of the tile: row (lane >> 4) + 4 reg, column lane & 15
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) v += tile_s[w][tid];
        a.part_scatter[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + tid] = v;
    }
    if (diag && tid < 16) {
        double v = 0.0;
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int q = 0; q < 4; ++q) v += sum_s[w][q * 16 + tid];
        a.part_sum[((size_t)blockIdx.y * nt + ti) * 16 + tid] = v;
    }
}

__global__ void __launch_bounds__(256)
k_pooled_final(PooledArgs a) {
    const int d = a.d, nt = a.nt, ntile = nt * (nt + 1) / 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int nsc = a.want_scatter ? d * d : 0;
    if (idx >= nsc + d) return;
    if (idx >= nsc) {
        const int i = idx - nsc;
        double v = 0.0;
        for (int sl = 0; sl < a.nslab; ++sl) v += a.part_sum[(size_t)sl * nt * 16 + i];
        a.out_sum[i] = v;
        return;
    }
    const int i = idx % d, j = idx / d;
    if (i > j) return;                                          // written as the mirror image of (j, i)
    const int ti = i >> 4, tj = j >> 4, row = i & 15, col = j & 15;
    const int tile = ti * nt - ti * (ti - 1) / 2 + (tj - ti);
    const int e = (row >> 2) * 64 + (row & 3) * 16 + col;
    double v = 0.0;
    for (int sl = 0; sl < a.nslab; ++sl) v += a.part_scatter[((size_t)sl * ntile + tile) * 256 + e];
    a.out_scatter[i + (size_t)j * d] = v;
    a.out_scatter[j + (size_t)i * d] = v;
}

}  // namespace epx
