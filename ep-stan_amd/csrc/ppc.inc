// Posterior predictive checks of the context's OWN rows (include/epx.h, enum epx_ppc, states the definition; ppc.ppc_host
// restates it in NumPy).  Included by predict.hip, inside namespace epx, behind k_loo.
//
// k_predict and k_loo reduce over draws per row; a check reduces over ROWS per draw and only then over draws.
//
// k_ppc.  A work item is a whole (site, group): the workgroup walks the group's rows in items of 64 (a tile of 16 rows
// per wave) and, per item, the site's draws in slabs of 16 -- ONE pass of the row-tile walk of predict_tile.h over
// k_predict's slabs (predict_stage).  A lane holds the four cells (row kq + 4 r, draw lane & 15) of a slab step: the walk
// leaves it f, sigmoid(f) and ll(y) of each; in front of the slab's closing barrier it takes them one at a time (a rolled
// loop: the stream and the link once in registers, next to the tile), draws the cell's replicate from the samplers' Philox
// stream at kind K_PPC (a function of (seed, row, draw) alone), forms the log-likelihood of the replicate, and adds the
// three values y_rep, ll(y), ll(y_rep) over its r, then across the four kq lane groups of the wave (two permute steps:
// (kq 0 + 1) + (2 + 3)).  The waves' per-draw partial sums
// meet in LDS (part) and 48 threads add them in wave order onto acc[3][S], which carries over the items of the group.
// ll(y) and ll(y_rep) go through the same code in the same order: where y_rep = y on every row the two sums are equal
// to the bit.  No floating-point atomics; nothing is merged across workgroups, so no result depends on the grid.  Behind
// the last item the 3 x S per-draw values go to the workspace (k_ppc_sites and the optional export read them) and 16
// lanes reduce them to the group's record (ppc_record: two passes, row16_sum).
// k_ppc_sites.  16 lanes per site add the groups' per-draw values in group order and reduce them by the same ppc_record.

// the replicate of (row, draw s) at linear predictor f: mu = sigmoid(f), sg = sigma of the draw
__device__ inline double ppc_replicate(int gauss, RngKey key, uint32_t s, uint32_t row, double f, double mu, double sg) {
    if (gauss) return f + sg * rng_normal(key, s, K_PPC, (int)row, 0);
    return rng_uniform(key, s, K_PPC, row, 0) < mu ? 1.0 : 0.0;
}

// element r of a lane's four results, r not known to the compiler: a select, not an indexed register
template <class T>
__device__ __forceinline__ T ppc_pick(const T (&v)[4], int r) {
    return r == 0 ? v[0] : r == 1 ? v[1] : r == 2 ? v[2] : v[3];
}

// The record of a unit from its per-draw values val(q, s), q = 0: T_rep, 1: D_obs, 2: D_rep, by the 16 lanes c of a DPP
// row (t_obs and bad are the same in all of them): a lane adds its draws s = c, c + 16, ... in order, then row16_sum;
// the centred sum of squares in a second pass.
template <class V>
__device__ inline void ppc_record(V val, int S, double t_obs, bool bad, double *o, int c) {
    if (bad) {
        if (c < EPX_PC_COUNT) o[c] = NAN;
        return;
    }
    double st = 0.0, ge = 0.0, gt = 0.0, so = 0.0, sr = 0.0, le = 0.0;
    for (int s = c; s < S; s += 16) {
        const double t = val(0, s), d_obs = val(1, s), d_rep = val(2, s);
        st += t;
        ge += t >= t_obs ? 1.0 : 0.0;
        gt += t > t_obs ? 1.0 : 0.0;
        so += d_obs;
        sr += d_rep;
        le += d_rep <= d_obs ? 1.0 : 0.0;
    }
    const double mean = row16_sum(st) / (double)S;
    ge = row16_sum(ge);
    gt = row16_sum(gt);
    so = row16_sum(so);
    sr = row16_sum(sr);
    le = row16_sum(le);
    double q = 0.0;
    for (int s = c; s < S; s += 16) {
        const double dt = val(0, s) - mean;
        q += dt * dt;
    }
    q = row16_sum(q);
    if (c == 0) {
        o[EPX_PC_T_OBS] = t_obs;
        o[EPX_PC_T_MEAN] = mean;
        o[EPX_PC_T_M2] = q;
        o[EPX_PC_T_GE] = ge;
        o[EPX_PC_T_GT] = gt;
        o[EPX_PC_D_OBS_MEAN] = so / (double)S;
        o[EPX_PC_D_REP_MEAN] = sr / (double)S;
        o[EPX_PC_D_LE] = le;
    }
}

// EPX_PPC_WAVES: the waves per SIMD the compiler has to leave room for.  2 caps the kernel at 256 registers (29 of them
// spilled) and lets two workgroups share a compute unit: 1.5 times faster at the C3 shape than the 296 registers and one
// workgroup of an uncapped build (A/B: make variant ... EXTRA=-DEPX_PPC_WAVES=1; DESIGN.md, section 3.2)
#ifndef EPX_PPC_WAVES
#define EPX_PPC_WAVES 2
#endif
__global__ void __launch_bounds__(256, EPX_PPC_WAVES)
k_ppc(PpcArgs a) {
    extern __shared__ __attribute__((aligned(16))) double ppc_lds[];
    const PredictArgs &p = a.p;
    const Slab sl{ppc_lds, ppc_lds + p.m.KP * 16, ppc_lds + p.m.KP * 16 + 16};
    double *part = sl.sig + 16, *scr = part + EPX_PC_WAVE_PART;
    int *flag = reinterpret_cast<int *>(scr + 16);
    double *acc = scr + 18;                                // ppc_fixed_doubles(KP) in front of it
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int S = p.S, gauss = p.m.gauss, nstep = p.m.KP / 4;
    const int t0 = wave * EPX_PR_TILE;
    const RngKey key = make_key(a.seed, 0);

    for (int wi = blockIdx.x; wi < a.ngroups; wi += gridDim.x) {
        const PredictWg w = p.wg[wi];
        const int k = p.k0 + w.site, g = w.group;
        const int ng = p.site_g0 ? p.site_g0[k + 1] - p.site_g0[k] : 1;
        const double *TH = p.draws + (size_t)w.site * S * p.m.P;
        const auto y_of = [&](size_t row) { return gauss ? a.yd[row] : (double)a.y8[row]; };

        for (int i = tid; i < 3 * S; i += 256) acc[i] = 0.0;
        if (tid == 0) *flag = 0;
        double ty = 0.0;
        for (int i = tid; i < w.rows; i += 256) ty += y_of((size_t)w.first + i);
        // (its barriers also stand between the zeroes above and the first slab's sums)
        const double t_obs = wg_reduce(row16_sum(ty), scr, [](double x, double y) { return x + y; });

        bool bad = false;
        for (int rb = 0; rb < w.rows; rb += EPX_PR_WG_ROWS) {
            const int first = w.first + rb, rows = w.rows - rb < EPX_PR_WG_ROWS ? w.rows - rb : (int)EPX_PR_WG_ROWS;
            const bool busy = t0 < rows;                  // (wave-uniform: a wave without rows only stages)
            RowTile t;
            tile_load(t, p.X, p.m.D, nullptr, first, rows, t0, busy, true, y_of);
            for (int s0 = 0; s0 < S; s0 += 16) {
                const bool in = s0 + col < S;
                double fv[4] = {}, mv[4] = {}, lv[4] = {};      // the lane's four cells: f, sigmoid(f), ll(y)
                tile_slab(t, sl, gauss, nstep, busy, in, true, [&] { predict_stage(p, TH, s0, g, ng, sl); },
                          [&](int r, double f, double mu, double ll) { fv[r] = f; mv[r] = mu; lv[r] = ll; },
                          [&] {                           // all threads, in front of the slab's closing barrier
                              // the lane's sums over its rows r = 0..3, in order: y_rep, ll(y), ll(y_rep).  One cell
                              // at a time (the loop stays rolled: one copy of the stream and the link in registers)
                              double lt = 0.0, lo = 0.0, lr = 0.0;
                              if (busy && in) {
                                  const double ls = gauss ? sl.lsig[col] : 0.0, sg = gauss ? sl.sig[col] : 1.0;
#pragma unroll 1
                                  for (int r = 0; r < 4; ++r) {
                                      const int row = ppc_pick(t.row, r);
                                      if (row < 0) continue;
                                      const double f = ppc_pick(fv, r), ll = ppc_pick(lv, r);
                                      const double yr = ppc_replicate(gauss, key, (uint32_t)(s0 + col),
                                                                      (uint32_t)(a.row0 + row), f, ppc_pick(mv, r), sg);
                                      double mu_r, ll_r;
                                      predict_link(gauss, f, yr, ls, sg, mu_r, ll_r);
                                      lt += yr;
                                      lo += ll;
                                      lr += ll_r;
                                      bad |= !(isfinite(f) && isfinite(ll) && isfinite(ll_r));
                                  }
                              }
                              // the wave's 16 rows of every column: the four kq lane groups, then LDS
                              lt += __shfl_xor(lt, 16); lt += __shfl_xor(lt, 32);
                              lo += __shfl_xor(lo, 16); lo += __shfl_xor(lo, 32);
                              lr += __shfl_xor(lr, 16); lr += __shfl_xor(lr, 32);
                              if (kq == 0) {
                                  part[(wave * 3 + 0) * 16 + col] = lt;
                                  part[(wave * 3 + 1) * 16 + col] = lo;
                                  part[(wave * 3 + 2) * 16 + col] = lr;
                              }
                          });
                // value tid >> 4 of draw s0 + (tid & 15): the four waves in order.  (The next slab's partial sums are
                // written behind its first barrier.)
                if (tid < 48 && s0 + (tid & 15) < S) {
                    const int q = tid >> 4;
                    double s = part[q * 16 + (tid & 15)];
                    for (int v = 1; v < 4; ++v) s += part[(v * 3 + q) * 16 + (tid & 15)];
                    acc[q * S + s0 + (tid & 15)] += s;
                }
            }
        }
        if (bad) atomicOr(flag, 1);
        __syncthreads();
        double *ws = a.per_draw + (size_t)wi * 3 * S;
        for (int i = tid; i < 3 * S; i += 256) ws[i] = acc[i];
        if (tid < 16)
            ppc_record([&](int q, int s) { return acc[q * S + s]; }, S, t_obs, *flag != 0,
                       a.out_groups + (size_t)wi * EPX_PC_COUNT, tid);
        __syncthreads();                                  // the next group zeroes acc and the flag
    }
}

__global__ void __launch_bounds__(256)
k_ppc_sites(PpcArgs a) {
    const int tid = threadIdx.x, c = tid & 15, S = a.p.S;
    for (int j = blockIdx.x * 16 + (tid >> 4); j < a.count; j += gridDim.x * 16) {
        const int g0 = a.site_first[j], g1 = a.site_first[j + 1];
        bool bad = false;                                 // (a group's record is NaN in all columns or in none)
        double t_obs = 0.0;
        for (int g = g0; g < g1; ++g) {
            const double v = a.out_groups[(size_t)g * EPX_PC_COUNT + EPX_PC_T_OBS];
            bad |= isnan(v);
            t_obs = g == g0 ? v : t_obs + v;
        }
        ppc_record([&](int q, int s) {
                       double v = 0.0;
                       for (int g = g0; g < g1; ++g) {
                           const double x = a.per_draw[((size_t)g * 3 + q) * S + s];
                           v = g == g0 ? x : v + x;
                       }
                       return v;
                   }, S, t_obs, bad, a.out_sites + (size_t)j * EPX_PC_COUNT, c);
    }
}
