// Order statistics across the draws of NEW rows (include/epx.h, enum epx_pred_order, states the definition;
// predict_quantiles.predict_order_stats_host restates it in NumPy): what Master.predict_quantiles interpolates into the
// credible band of a row's linear predictor or fitted probability and into the predictive interval of its response.
// Included by predict.hip, inside namespace epx, behind ppc.inc (ppc_pick).
//
// k_predict_order.  A work item is up to R rows of ONE (site, group), R in {16, 8, 4, 2, 1} (the host sizes it: R x N
// keys of 8 bytes have to fit the LDS behind the walk's fixed part, N = S rounded up to a power of two).  Per item:
//   1. the value tile.  All four waves hold the item's rows as their tile and share the site's draws: a step of the walk
//      stages FOUR of k_predict's slabs (predict_stage: 64 draws) and wave w takes slab w -- ONE pass of the row-tile
//      walk (predict_tile.h: tile_load, tile_slab) in a quarter of the steps, each with its two barriers and its exposed
//      load of the draws, and on all four matrix pipes.  In front of a step's closing barrier a lane takes its four
//      cells (row kq + 4 r, draw 16 w + lane & 15 of the step) one at a time (a rolled loop, as k_ppc's), forms v = f or,
//      for EPX_PO_YREP, f + sigma z with z from the samplers' stream at kind K_PRED_REP (a function of (seed, row_id,
//      draw) alone), and writes order_key(v) to the row's key s.  The 16 lanes of a kq group write 16 consecutive keys
//      of one row (at po_at, below: still 16 different slots of 8 bytes), 32 different banks; the kq groups write the
//      same columns of different rows, a multiple of 256 bytes apart.  IF a ds_write_b64 is served in groups of 16
//      contiguous lanes, the store is free of conflicts; served in halves of 32 lanes it is 2-way.  Not measured:
//      SQ_LDS_BANK_CONFLICT was not collected.  Behind S a row holds ORDER_KEY_PAD; a NaN sets the row's flag.
//   2. the sort.  The bitonic network of k_site_order_stats (quantiles.inc) on every row at once, up to THREE distances
//      of a merge per pass through the LDS: a thread owns the 8 keys base + m js, m < 8, of a row (js the smallest of
//      the pass's distances), holds them in registers and does the exchanges at 4 js, 2 js and js there -- all pairs of
//      those distances lie inside such a group.  The passes of a merge are grouped from the bottom, so js is a power of
//      8: 22 passes and barriers at N = 1024 where one distance per pass takes 55, and a thread's 8 loads are in flight
//      together (one workgroup per CU at R = 16: nothing else hides their latency).  The groups of a pass are dealt to
//      the 256 threads in one index space, group -> (row, group of the row): all threads work whatever R is, and the
//      trip counts and barriers depend on (rows, N) alone.
//      Banks.  Key i of a row lies at po_at(i) = i ^ ((i >> 5) & 7) ^ (((i >> 6) & 3) << 3): bits 5..7 folded into bits
//      0..2 and bits 6..7 into bits 3..4, a permutation of every aligned 32 keys (one 256-byte bank row).  Straight, the
//      32 lanes of a ds_read_b64 at js = 1 (lane l reads key 8 l + m) would meet on 4 bank slots, 8-way, and at js = 8
//      (64 (l >> 3) + (l & 7) + 8 m) on 8, 4-way; folded, both hit 32 different slots, and so do 32 consecutive keys (js
//      >= 64).  Computed from the bank rule (bank = byte address / 4 mod 64 for an 8-byte read, lanes in halves of 32)
//      and checked by enumeration, not measured; the stores of the js = 1 pass stay 2-way even in 16-lane groups.
//      A sort of keys has ONE result, whatever the network: the same bits as quantiles.order_stats.
//   3. the output.  The asked ranks of every row as doubles, NaN where the row's flag is set; a barrier in front of the
//      next item, which overwrites the tile.
// No floating-point atomics, no atomics at all; nothing is merged across workgroups: a row's result does not depend on
// the grid, the sub-range of sites or the other rows of the call.

// where key i of a row lies in the row (see "Banks" above); i < N, and the row keeps its N slots
__device__ __forceinline__ int po_at(int i) { return i ^ ((i >> 5) & 7) ^ (((i >> 6) & 3) << 3); }

__device__ __forceinline__ void po_exchange(unsigned long long &lo, unsigned long long &hi, bool up) {
    if ((lo > hi) == up) { const unsigned long long t = lo; lo = hi; hi = t; }
}

// One pass of merge kk over rows [0, rows) of N = 1 << lg keys: the ND distances j, j / 2, ..., js = j >> (ND - 1)
template <int ND>
__device__ __forceinline__ void po_pass(unsigned long long *keys, int rows, int lg, int kk, int j) {
    constexpr int C = 1 << ND;
    const int js = j >> (ND - 1), ngrp = rows << (lg - ND);
    for (int q = threadIdx.x; q < ngrp; q += 256) {
        const int i = q & ((1 << (lg - ND)) - 1);
        const int base = ((i & ~(js - 1)) << ND) | (i & (js - 1));      // ND zero bits at js: the group's first key
        unsigned long long *row = keys + ((size_t)(q >> (lg - ND)) << lg);
        const bool up = (base & kk) == 0;                  // (kk lies above every bit the group spans)
        unsigned long long v[C];
#pragma unroll
        for (int m = 0; m < C; ++m) v[m] = row[po_at(base + m * js)];
#pragma unroll
        for (int d = C / 2; d >= 1; d >>= 1) {
#pragma unroll
            for (int m = 0; m < C; ++m)
                if ((m & d) == 0) po_exchange(v[m], v[m + d], up);
        }
#pragma unroll
        for (int m = 0; m < C; ++m) row[po_at(base + m * js)] = v[m];
    }
    __syncthreads();
}

// Sorts rows [0, rows) of 1 << lg keys each, row rr at keys + (rr << lg), ascending; all 256 threads, barriers inside.
// Merge kk = 2^L has the L distances kk / 2 ... 1: first the (L - 1) mod 3 + 1 largest, then three at a time.
__device__ inline void po_sort_rows(unsigned long long *keys, int rows, int lg) {
    for (int L = 1; L <= lg; ++L) {
        const int kk = 1 << L;
        int nd = (L - 1) % 3 + 1;
        for (int j = kk >> 1; j > 0; j >>= nd, nd = 3) {
            if (nd == 3) po_pass<3>(keys, rows, lg, kk, j);
            else if (nd == 2) po_pass<2>(keys, rows, lg, kk, j);
            else po_pass<1>(keys, rows, lg, kk, j);
        }
    }
}

__global__ void __launch_bounds__(256)
k_predict_order(PredOrderArgs a) {
    extern __shared__ __attribute__((aligned(16))) double po_lds[];
    const PredictArgs &p = a.p;
    const int slab_doubles = p.m.KP * 16 + 32;            // a slab: coefficients, log sigma, sigma
    const auto slab_of = [&](int q) {
        double *at = po_lds + q * slab_doubles;
        return Slab{at, at + p.m.KP * 16, at + p.m.KP * 16 + 16};
    };
    int *flag = reinterpret_cast<int *>(po_lds + 4 * slab_doubles);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(po_lds + 4 * slab_doubles + 8);   // pred_order_fixed_bytes(KP) in front
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int S = p.S, N = a.npad, gauss = p.m.gauss, nstep = p.m.KP / 4;
    const bool yrep = a.what == EPX_PO_YREP;
    const RngKey key = make_key(a.seed, 0);

    for (int wi = blockIdx.x; wi < a.nwg; wi += gridDim.x) {
        const PredictWg w = p.wg[wi];
        const int k = p.k0 + w.site, g = w.group;
        const int ng = p.site_g0 ? p.site_g0[k + 1] - p.site_g0[k] : 1;
        const double *TH = p.draws + (size_t)w.site * S * p.m.P;
        const bool busy = true;                           // (every wave holds the item's one tile, for its own slab of a step)

        if (tid < 16) flag[tid] = 0;
        for (int rr = 0; rr < w.rows; ++rr)
            for (int i = S + tid; i < N; i += 256) keys[((size_t)rr << a.lg) + po_at(i)] = ORDER_KEY_PAD;
        RowTile t;
        tile_load(t, p.X, p.m.D, p.perm, w.first, w.rows, 0, busy, false, [](size_t) { return 0.0; });
        uint32_t eid[4];                                  // the stream's index of the lane's four rows
#pragma unroll
        for (int r = 0; r < 4; ++r)
            eid[r] = t.row[r] < 0 ? 0u : a.row_id ? a.row_id[t.row[r]] : (uint32_t)t.row[r];
        // (the first slab's opening barrier stands between the flags and pads above and the cells below)
        const Slab sl = slab_of(wave);
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int s = s0 + 16 * wave + col;           // the lane's draw
            const bool in = s < S;
            double fv[4] = {};
            tile_slab(t, sl, gauss, nstep, busy, in, false,
                      [&] { for (int q = 0; q < 4; ++q) predict_stage(p, TH, s0 + 16 * q, g, ng, slab_of(q)); },
                      [&](int r, double f, double, double) { fv[r] = f; },
                      [&] {                               // all threads, in front of the slab's closing barrier
                          if (busy && in) {
                              const double sg = yrep ? sl.sig[col] : 0.0;
#pragma unroll 1
                              for (int r = 0; r < 4; ++r) {
                                  if (ppc_pick(t.row, r) < 0) continue;
                                  double v = ppc_pick(fv, r);
                                  if (yrep) v = v + sg * rng_normal(key, (uint32_t)s, K_PRED_REP, (int)ppc_pick(eid, r), 0);
                                  const int rr = kq + 4 * r;
                                  keys[((size_t)rr << a.lg) + po_at(s)] = order_key(v);
                                  if (v != v) flag[rr] = 1;
                              }
                          }
                      });
        }
        po_sort_rows(keys, w.rows, a.lg);
        for (int o = tid; o < w.rows * a.n_ranks; o += 256) {
            const int rr = o / a.n_ranks, q = o - rr * a.n_ranks;
            const size_t row = (size_t)p.perm[w.first + rr];
            a.out[row * a.n_ranks + q] = flag[rr] ? __builtin_nan("") : order_value(keys[((size_t)rr << a.lg) + po_at(a.rank[q])]);
        }
        __syncthreads();                                  // the next item overwrites the tile and the flags
    }
}
