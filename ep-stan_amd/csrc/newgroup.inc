// Posterior predictive of a group that was NOT in the data (include/epx.h: epx_predict_new_group states the definition;
// newgroup.py restates it in NumPy).  Included by predict.hip, inside namespace epx, behind k_predict's stage helpers.
//
// The pool: N = count x S x R members m = (b S + s) R + r, draw s of site b of the call with replicate r of the new
// group's own latents; only phi (the first d coordinates of the draw record) is read.  The latents come from the
// samplers' Philox stream at kind K_NEWGROUP, keyed by the group's label: a function of (seed, label, t, r, e) alone.
//
// k_newgroup.  A work item is (new group, chunk of the pool): chunks are newgroup_chunk_slabs(N) slabs of 16 members, a
// function of N alone.  The workgroup walks the group's rows in blocks of 64 and, per block, the chunk's slabs twice:
// the row-tile walk of predict_tile.h, a slab column being a pool member.  This file adds where a slab comes from
// (newgroup_stage): a thread = (member tid & 15, Box-Muller / Laplace pair tid >> 4, + 16, ...) draws the pair's two
// latents and writes coef[k][member] by named_elem_of's transforms at one group, the latent in the place of the sampled
// eta / etb.  And, with responses, what pass 1 does beside the walk's sums: the sum of ll over the block's rows per
// member, lane -> LDS -> 16 threads add the 16 partial sums of a member (4 waves x 4 row quarters) in a fixed order onto
// gll[member], block after block: the group's JOINT log-likelihood under the member's shared latents.  Pass 2
// regenerates the slabs (the same bits: the stream is counter-based).  The row's chunk record [mean, f mean, M2,
// log-mean-exp] goes to the workspace; behind the last block the 256 threads reduce gll to the chunk's log-mean-exp of
// the joint term.
// k_newgroup_merge adds the chunk records of a row, or of a group, in ascending chunk order with the merge rules of the
// definition.  No atomics anywhere; the bits of a row's record depend on the row, the group's label and the pool only,
// those of a group's joint term on the group's rows in the call's order.

__device__ inline double newgroup_laplace(double u) {
    const double x = u - 0.5;
    return copysign(-log1p(-2.0 * fabs(x)), x);         // -sign(x) log1p(-2 |x|)
}

// latents 2 p and 2 p + 1 of pooled draw t, replicate r
__device__ inline void newgroup_pair(RngKey key, uint32_t t, uint32_t r, int p, int lap, double &z0, double &z1) {
    double u1, u2;
    rng_u2(key, t, K_NEWGROUP, (uint32_t)p, r, u1, u2);
    if (lap) {
        z0 = newgroup_laplace(u1);
        z1 = newgroup_laplace(u2);
    } else {                                             // rng_normal's pair
        const double rad = sqrt(-2.0 * log(u1));
        double s, c;
        sincos(6.283185307179586476925286766559 * u2, &s, &c);
        z0 = rad * c;
        z1 = rad * s;
    }
}

// named_value with the latent z in the place of the sampled eta / etb (th[el.ia]); m1's beta is part of phi
__device__ inline double newgroup_value(const NamedElem &el, const double *th, double z) {
    switch (el.kind) {
    case NM_ID: return th[el.ia];
    case NM_MUL: return z * exp_d(th[el.ib]);
    case NM_MULADD: return th[el.ic] + z * exp_d(th[el.ib]);
    default: return 0.0;
    }
}

// The coefficient block of the slab of members m0 .. m0 + 15 (those below m_hi)
__device__ inline void newgroup_stage(const NewGroupArgs &a, RngKey key, long long m0, long long m_hi, const Slab &sl) {
    const int tid = threadIdx.x, c = tid & 15;
    const long long m = m0 + c;
    const bool in = m < m_hi;
    const long long bs = in ? m / a.R : 0;               // site-major draw of the call
    const uint32_t r = (uint32_t)(in ? m - bs * a.R : 0), t = (uint32_t)(a.t0 + bs);
    const double *th = a.draws + (size_t)bs * a.m.P;
    for (int p = tid >> 4; 2 * p < a.m.KP; p += 16) {
        double z[2] = {0.0, 0.0};
        if (in && 2 * p < a.E) newgroup_pair(key, t, r, p, a.lap, z[0], z[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * p + h;
            double v = 0.0;
            if (in && k <= a.m.D) v = newgroup_value(tile_coef_elem(a.m, k, 0, 1), th, z[h]);
            sl.coef[k * 16 + c] = v;
        }
    }
    tile_stage_scale(a.m, th, in, sl.lsig, sl.sig);
}

__global__ void __launch_bounds__(256)
k_newgroup(NewGroupArgs a) {
    __shared__ double coef[PR_KMAX * 16];
    __shared__ double lsig[16], sig[16], scr[16];
    __shared__ double part[256];                          // pass 1: a lane's sum of ll over its rows, per slab
    __shared__ double gll[EPX_NGP_MAX_SLABS * 16];        // the chunk's members: sum of ll over the group's rows
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int gauss = a.m.gauss, nstep = a.m.KP / 4;
    const int t0 = wave * EPX_PR_TILE;
    const bool has_y = a.y != nullptr;
    const long long chunk = (long long)a.chunk_slabs * 16;
    const Slab sl{coef, lsig, sig};

    for (long long wi = blockIdx.x; wi < a.nitem; wi += gridDim.x) {
        const int g = a.live[wi / a.nchunk];
        const long long ch = wi % a.nchunk;
        const long long m_lo = ch * chunk, m_hi = m_lo + chunk < a.N ? m_lo + chunk : a.N;
        const double Nc = (double)(m_hi - m_lo);
        const int gfirst = a.gfirst[g], grows = a.gfirst[g + 1] - gfirst;
        const RngKey key = make_key(a.seed, a.label[g]);
        for (int i = tid; i < a.chunk_slabs * 16; i += 256) gll[i] = 0.0;

        for (int rb = 0; rb < grows; rb += EPX_PR_WG_ROWS) {
            const int first = gfirst + rb, rows = grows - rb < EPX_PR_WG_ROWS ? grows - rb : (int)EPX_PR_WG_ROWS;
            const bool busy = t0 < rows;                  // (wave-uniform: a wave without rows only stages)
            RowTile t;
            tile_load(t, a.X, a.m.D, a.perm, first, rows, t0, busy, has_y, [&](size_t row) { return a.y[row]; });
            RowSums sums;
            sums_begin(sums);
            // ---- pass 1, and the members' sums of ll over the block's rows onto gll
            for (long long m0 = m_lo; m0 < m_hi; m0 += 16) {
                double lsum = 0.0;
                tile_slab(t, sl, gauss, nstep, busy, m0 + col < m_hi, true, [&] { newgroup_stage(a, key, m0, m_hi, sl); },
                          [&](int r, double f, double mu, double ll) {
                              sums_add1(sums, r, f, mu, ll);
                              if (t.row[r] >= 0) lsum += ll;
                          },
                          [&] { if (has_y) part[tid] = lsum; });
                if (has_y && tid < 16) {                  // member tid of the slab: waves 0..3, row quarters 0..3, in order
                    double s = 0.0;
                    for (int i = 0; i < 16; ++i) s += part[i * 16 + tid];
                    gll[(int)(m0 - m_lo) + tid] += s;
                }
            }
            sums_close1(sums, Nc);
            // ---- pass 2; the row's chunk record goes to its sorted position
            for (long long m0 = m_lo; m0 < m_hi; m0 += 16)
                tile_slab(t, sl, gauss, nstep, busy, m0 + col < m_hi, has_y, [&] { newgroup_stage(a, key, m0, m_hi, sl); },
                          [&](int r, double f, double mu, double ll) { sums_add2(sums, r, f, ll, has_y); }, [] {});
            sums_close2(sums, t, Nc, has_y, [&](int r) {
                return a.part_rows + ((size_t)ch * a.n + first + t0 + kq + 4 * r) * EPX_PR_COUNT;
            });
        }

        // ---- the group's joint term of the chunk: log-mean-exp of gll about its largest entry
        if (has_y) {
            __syncthreads();
            const int nm = (int)(m_hi - m_lo);
            double top = -INFINITY;
            for (int i = tid; i < nm; i += 256) top = fmax(top, gll[i]);
            top = wg_reduce(row16_max(top), scr, [](double x, double y) { return fmax(x, y); });
            double s = 0.0;
            for (int i = tid; i < nm; i += 256) s += exp_d(gll[i] - top);
            s = wg_reduce(row16_sum(s), scr, [](double x, double y) { return x + y; });
            if (tid == 0) a.part_grp[(size_t)ch * a.G + g] = top + log_pos_d(s / Nc);
        }
        __syncthreads();                                  // the next item zeroes gll
    }
}

// log-mean-exp of the union of two pools of Na and Nb members from theirs: logaddexp(a + log Na, b + log Nb) - log N,
// written about the larger of the two (equal inputs come back as they are)
__device__ inline double newgroup_merge_lme(double la, double Na, double lb, double Nb) {
    const double top = fmax(la, lb);
    if (isnan(la) || isnan(lb)) return NAN;
    return top + log((Na * exp(la - top) + Nb * exp(lb - top)) / (Na + Nb));
}

// One thread per row (sorted position i < n) or group (n + g): the chunk records in ascending chunk order
__global__ void __launch_bounds__(256)
k_newgroup_merge(NewGroupArgs a) {
    const long long chunk = (long long)a.chunk_slabs * 16;
    const bool has_y = a.y != nullptr;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < (long long)a.n + a.G; i += (long long)gridDim.x * 256) {
        if (i < a.n) {
            double Na = 0.0, mean = 0.0, fmean = 0.0, m2 = 0.0, lpd = 0.0;
            for (long long ch = 0; ch < a.nchunk; ++ch) {
                const long long m_lo = ch * chunk;
                const double Nb = (double)((m_lo + chunk < a.N ? m_lo + chunk : a.N) - m_lo), N = Na + Nb;
                const double *p = a.part_rows + ((size_t)ch * a.n + i) * EPX_PR_COUNT;
                if (ch == 0) {
                    mean = p[EPX_PR_MEAN]; fmean = p[EPX_PR_F_MEAN]; m2 = p[EPX_PR_F_M2]; lpd = p[EPX_PR_LPD];
                } else {
                    const double dlt = fmean - p[EPX_PR_F_MEAN];
                    m2 = m2 + p[EPX_PR_F_M2] + dlt * dlt * (Na * Nb / N);
                    mean = (Na * mean + Nb * p[EPX_PR_MEAN]) / N;
                    fmean = (Na * fmean + Nb * p[EPX_PR_F_MEAN]) / N;
                    if (has_y) lpd = newgroup_merge_lme(lpd, Na, p[EPX_PR_LPD], Nb);
                }
                Na = N;
            }
            double *o = a.out + (size_t)a.perm[i] * EPX_PR_COUNT;
            o[EPX_PR_MEAN] = mean;
            o[EPX_PR_F_MEAN] = fmean;
            o[EPX_PR_F_M2] = m2;
            o[EPX_PR_LPD] = has_y ? lpd : NAN;
        } else {
            const int g = (int)(i - a.n);
            double v = NAN;
            if (has_y) {
                v = 0.0;                                  // a group without rows
                if (a.gfirst[g + 1] > a.gfirst[g]) {
                    double Na = 0.0;
                    for (long long ch = 0; ch < a.nchunk; ++ch) {
                        const long long m_lo = ch * chunk;
                        const double Nb = (double)((m_lo + chunk < a.N ? m_lo + chunk : a.N) - m_lo);
                        const double p = a.part_grp[(size_t)ch * a.G + g];
                        v = ch == 0 ? p : newgroup_merge_lme(v, Na, p, Nb);
                        Na += Nb;
                    }
                }
            }
            a.out_group[(size_t)g * EPX_NG_COUNT + EPX_NG_GLPD] = v;
        }
    }
}

// TEST HOOK: the latents themselves, out (nt, R, E); a thread per (pooled draw, replicate, pair)
__global__ void __launch_bounds__(256)
k_newgroup_latents(uint64_t seed, int label, long long t0, long long nt, int R, int E, int lap, double *out) {
    const RngKey key = make_key(seed, label);
    const int np = (E + 1) / 2;
    const long long total = nt * R * np;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int p = (int)(i % np);
        const long long tr = i / np, ti = tr / R;
        const uint32_t r = (uint32_t)(tr - ti * R);
        double z0, z1;
        newgroup_pair(key, (uint32_t)(t0 + ti), r, p, lap, z0, z1);
        double *o = out + (size_t)tr * E + 2 * p;
        o[0] = z0;
        if (2 * p + 1 < E) o[1] = z1;
    }
}
