// Posterior predictive of a group that was NOT in the data (include/epx.h: epx_predict_new_group states the definition;
// newgroup.py restates it in NumPy).  Included by predict.hip, inside namespace epx, behind k_predict's stage helpers.
//
// The pool: N = count x S x R members m = (b S + s) R + r, draw s of site b of the call with replicate r of the new
// group's own latents; only phi (the first d coordinates of the draw record) is read.  The latents come from the
// samplers' Philox stream at kind K_NEWGROUP, keyed by the group's label: a function of (seed, label, t, r, e) alone.
//
// k_newgroup.  A work item is (new group, chunk of the pool): chunks are newgroup_chunk_slabs(N) slabs of 16 members, a
// function of N alone.  The workgroup walks the group's rows in blocks of 64 (a tile of 16 per wave, the A operand in
// registers as in k_predict) and, per block, the chunk's slabs twice:
//   - all 256 threads stage the slab: a thread = (member tid & 15, Box-Muller / Laplace pair tid >> 4, + 16, ...) draws
//     the pair's two latents and writes coef[k][member], k = 0 alpha, k = 1 + j beta_j (named_elem_of's transforms at
//     one group, the latent in the place of the sampled eta / etb), zeros behind 1 + D and behind the last member;
//   - every wave multiplies its row tile by the slab (predict_product) and applies predict_link.
// Pass 1: chunk-local sums of f and of the link's value, the largest ll of every row -- and, with responses, the sum of
// ll over the block's rows per member: lane -> LDS -> 16 threads add the 16 partial sums of a member (4 waves x 4 row
// quarters) in a fixed order onto gll[member], block after block: the group's JOINT log-likelihood under the member's
// shared latents.  Pass 2 regenerates the slabs (the same bits: the stream is counter-based) for the centred squares
// and sum exp(ll - max).  The row's chunk record [mean, f mean, M2, log-mean-exp] goes to the workspace; behind the
// last block the 256 threads reduce gll to the chunk's log-mean-exp of the joint term.
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
__device__ inline void newgroup_stage(const NewGroupArgs &a, RngKey key, long long m0, long long m_hi, double *coef,
                                      double *lsig, double *sig) {
    const int tid = threadIdx.x, c = tid & 15;
    const long long m = m0 + c;
    const bool in = m < m_hi;
    const long long bs = in ? m / a.R : 0;               // site-major draw of the call
    const uint32_t r = (uint32_t)(in ? m - bs * a.R : 0), t = (uint32_t)(a.t0 + bs);
    const double *th = a.draws + (size_t)bs * a.P;
    for (int p = tid >> 4; 2 * p < a.KP; p += 16) {
        double z[2] = {0.0, 0.0};
        if (in && 2 * p < a.E) newgroup_pair(key, t, r, p, a.lap, z[0], z[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * p + h;
            double v = 0.0;
            if (in && k <= a.D) {
                const NamedElem el = k == 0 ? named_elem_of(EPX_NM_ALPHA, 0, a.model, a.D, a.d, a.gauss, 1)
                                            : named_elem_of(EPX_NM_BETA, k - 1, a.model, a.D, a.d, a.gauss, 1);
                v = newgroup_value(el, th, z[h]);
            }
            coef[k * 16 + c] = v;
        }
    }
    if (a.gauss && tid < 16) {                           // y ~ normal(f, sigma), sigma = exp(phi[0])
        const double ls = in ? th[0] : 0.0;
        lsig[tid] = ls;
        sig[tid] = exp_d(ls);
    }
}

// max / sum over the workgroup of a value per thread, in a fixed order: 16 lanes by DPP, the 16 rows through LDS
__device__ inline double newgroup_wg_max(double v, double *scr) {
    v = row16_max(v);
    __syncthreads();
    if ((threadIdx.x & 15) == 0) scr[threadIdx.x >> 4] = v;
    __syncthreads();
    double o = scr[0];
    for (int i = 1; i < 16; ++i) o = fmax(o, scr[i]);
    return o;
}
__device__ inline double newgroup_wg_sum(double v, double *scr) {
    v = row16_sum(v);
    __syncthreads();
    if ((threadIdx.x & 15) == 0) scr[threadIdx.x >> 4] = v;
    __syncthreads();
    double o = scr[0];
    for (int i = 1; i < 16; ++i) o += scr[i];
    return o;
}

__global__ void __launch_bounds__(256)
k_newgroup(NewGroupArgs a) {
    __shared__ double coef[PR_KMAX * 16];
    __shared__ double lsig[16], sig[16], scr[16];
    __shared__ double part[256];                          // pass 1: a lane's sum of ll over its rows, per slab
    __shared__ double gll[EPX_NGP_MAX_SLABS * 16];        // the chunk's members: sum of ll over the group's rows
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int D = a.D, nstep = a.KP / 4;
    const int t0 = wave * EPX_PR_TILE;
    const bool has_y = a.y != nullptr;
    const long long chunk = (long long)a.chunk_slabs * 16;

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
            // A operand: lane = (row col, k kq) of every step; column 0 of the tile is the 1 that takes alpha
            double xa[PR_STEPS];
#pragma unroll
            for (int i = 0; i < PR_STEPS; ++i) xa[i] = 0.0;
            if (busy && t0 + col < rows) {
                const double *x = a.X + (size_t)a.perm[first + t0 + col] * D;
#pragma unroll
                for (int i = 0; i < PR_STEPS; ++i) {
                    const int c = 4 * i + kq;
                    if (c <= D) xa[i] = c == 0 ? 1.0 : x[c - 1];
                }
            }
            // results: lane = (rows kq + 4 r, member col)
            int srow[4];                                  // sorted position of the row, or -1
            double yv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tr = t0 + kq + 4 * r;
                srow[r] = busy && tr < rows ? first + tr : -1;
                yv[r] = has_y && srow[r] >= 0 ? a.y[a.perm[srow[r]]] : 0.0;
            }

            // ---- pass 1: sums of f and of the link's value, the largest ll; the members' sums of ll over the rows
            double sf[4] = {0.0, 0.0, 0.0, 0.0}, sm[4] = {0.0, 0.0, 0.0, 0.0};
            double mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            for (long long m0 = m_lo; m0 < m_hi; m0 += 16) {
                newgroup_stage(a, key, m0, m_hi, coef, lsig, sig);
                __syncthreads();
                double lsum = 0.0;
                if (busy) {
                    const v4d f = predict_product(xa, coef, nstep, lane);
                    if (m0 + col < m_hi) {
                        const double ls = a.gauss ? lsig[col] : 0.0, sg = a.gauss ? sig[col] : 1.0;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            double mu, ll;
                            predict_link(a.gauss, f[r], yv[r], ls, sg, mu, ll);
                            sf[r] += f[r];
                            sm[r] += mu;
                            mx[r] = fmax(mx[r], ll);
                            if (srow[r] >= 0) lsum += ll;
                        }
                    }
                }
                if (has_y) part[tid] = lsum;
                __syncthreads();
                if (has_y && tid < 16) {                  // member tid of the slab: waves 0..3, row quarters 0..3, in order
                    double s = 0.0;
                    for (int i = 0; i < 16; ++i) s += part[i * 16 + tid];
                    gll[(int)(m0 - m_lo) + tid] += s;
                }
            }
            double fm[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                fm[r] = row16_sum(sf[r]) / Nc;
                sm[r] = row16_sum(sm[r]) / Nc;
                mx[r] = row16_max(mx[r]);
            }

            // ---- pass 2: centred squares of f, sum exp(ll - max)
            double q[4] = {0.0, 0.0, 0.0, 0.0}, se[4] = {0.0, 0.0, 0.0, 0.0};
            for (long long m0 = m_lo; m0 < m_hi; m0 += 16) {
                newgroup_stage(a, key, m0, m_hi, coef, lsig, sig);
                __syncthreads();
                if (busy) {
                    const v4d f = predict_product(xa, coef, nstep, lane);
                    if (m0 + col < m_hi) {
                        const double ls = a.gauss ? lsig[col] : 0.0, sg = a.gauss ? sig[col] : 1.0;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double c = f[r] - fm[r];
                            q[r] += c * c;
                            if (has_y) {
                                double mu, ll;
                                predict_link(a.gauss, f[r], yv[r], ls, sg, mu, ll);
                                se[r] += exp_d(ll - mx[r]);
                            }
                        }
                    }
                }
                __syncthreads();
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                q[r] = row16_sum(q[r]);
                se[r] = row16_sum(se[r]);
                if (col == 0 && srow[r] >= 0) {
                    double *o = a.part_rows + ((size_t)ch * a.n + srow[r]) * EPX_PR_COUNT;
                    o[EPX_PR_MEAN] = sm[r];
                    o[EPX_PR_F_MEAN] = fm[r];
                    o[EPX_PR_F_M2] = q[r];
                    o[EPX_PR_LPD] = has_y ? mx[r] + log_pos_d(se[r] / Nc) : NAN;
                }
            }
        }

        // ---- the group's joint term of the chunk: log-mean-exp of gll about its largest entry
        if (has_y) {
            __syncthreads();
            const int nm = (int)(m_hi - m_lo);
            double top = -INFINITY;
            for (int i = tid; i < nm; i += 256) top = fmax(top, gll[i]);
            top = newgroup_wg_max(top, scr);
            double s = 0.0;
            for (int i = tid; i < nm; i += 256) s += exp_d(gll[i] - top);
            s = newgroup_wg_sum(s, scr);
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
