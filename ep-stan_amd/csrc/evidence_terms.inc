// The terms of the bridge-sampling evidence estimate (include/epx.h, epx_site_evidence, states the definition; evidence.hip
// holds the two kernels around this one and the overview).  Included by predict.hip, inside namespace epx, behind k_ppc: the
// site's log-likelihood goes through the row-tile walk of predict_tile.h, as every predictive kernel's does.
//
// k_ev_terms.  l1 of the N1 estimation draws and l2 of N2 = N1 proposal draws, in slabs of 16 columns.  A column is worked
//              on by the 16 lanes of a DPP row (four columns per wave): its record theta goes to LDS (a copy of the
//              draw, or m + L z with z from the samplers' Philox stream at kind K_BRIDGE), with the quadratic form of the
//              proposal density (a forward substitution for a draw, |z|^2 for a proposal draw), the cavity's quadratic
//              form and the latents' prior.  The log-likelihood of the site's rows then goes through the row-tile walk of
//              predict_tile.h, group by group, 64 rows at a time, the slab's coefficient columns formed from the
//              records in LDS; the rows are added per column as k_ppc adds them (ppc.inc): the lane's four, the four
//              lane groups of a wave by two permute steps, the four waves in wave order, the 64-row blocks in order.

__global__ void __launch_bounds__(256)
k_ev_terms(EvidenceArgs a) {
    extern __shared__ __attribute__((aligned(16))) double ev_lds[];
    const int P = a.m.P, d = a.m.d, D = a.m.D, KP = a.m.KP, gauss = a.m.gauss, Pp = evidence_stride(P);
    double *Lp = ev_lds, *mv = Lp + evidence_packed(P), *mu = mv + P, *th = mu + P, *w = th + 16 * Pp;
    const Slab sl{w + 16 * Pp, w + 16 * Pp + KP * 16, w + 16 * Pp + KP * 16 + 16};
    double *part = sl.sig + 16, *acc = part + 64, *base = acc + 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int cl = tid >> 4, c = tid & 15;                // stage A: column cl of the slab by the 16 lanes c of a DPP row
    const int j0 = blockIdx.x, k = a.k0 + j0, ng = ev_groups(a, k), Pk = ev_coords(a, k), N1 = a.N1;
    const int nstep = KP / 4, t0 = wave * EPX_PR_TILE, lap = a.m.model == EPX_M5B_SG;
    const double *TH = a.draws + (size_t)j0 * a.S * P;
    const double *fit = a.fit + (size_t)j0 * evidence_fit_doubles(P);
    const double *Om = a.cav_Om + (size_t)k * d * d;
    const RngKey key = make_key(a.seed, (int)(a.site0 + k));
    const auto y_of = [&](size_t row) { return gauss ? a.yd[row] : (double)a.y8[row]; };

    for (int i = tid; i < P; i += 256) mv[i] = fit[i];
    for (int i = tid; i < (int)evidence_packed(P); i += 256) Lp[i] = fit[P + i];
    for (int i = tid; i < d; i += 256) mu[i] = a.cav_mu[(size_t)k * d + i];
    const double sumlog = fit[P + evidence_packed(P)];
    __syncthreads();

    for (int set = 0; set < 2; ++set) {
        for (int c0 = 0; c0 < N1; c0 += 16) {
            // ---- stage A.  A column behind the last repeats the last one (its result is not used)
            const int e = c0 + cl < N1 ? c0 + cl : N1 - 1;
            double *tc = th + cl * Pp, *wc = w + cl * Pp;
            double quad = 0.0;
            if (set == 0) {
                const double *src = TH + (size_t)ev_est_draw(a, e) * P;
                for (int i = c; i < Pk; i += 16) tc[i] = src[i];
                psis_row_sync();
                for (int i = 0; i < Pk; ++i) {            // L v = theta - m, row by row; |v|^2 in every lane
                    const double *Li = Lp + ev_tri(i, 0);
                    double s = 0.0;
                    for (int j = c; j < i; j += 16) s += Li[j] * wc[j];
                    const double v = ((tc[i] - mv[i]) - row16_sum(s)) / Li[i];
                    if (c == 0) wc[i] = v;
                    quad += v * v;
                    psis_row_sync();
                }
            } else {
                double q = 0.0;
                for (int p = c; 2 * p < Pk; p += 16) {    // rng_normal's pair of elements 2 p, 2 p + 1
                    double u1, u2, sn, cs;
                    rng_u2(key, (uint32_t)e, K_BRIDGE, (uint32_t)p, 0, u1, u2);
                    const double rad = sqrt(-2.0 * log(u1));
                    sincos(6.283185307179586476925286766559 * u2, &sn, &cs);
                    const double z0 = rad * cs, z1 = rad * sn;
                    wc[2 * p] = z0;
                    q += z0 * z0;
                    if (2 * p + 1 < Pk) { wc[2 * p + 1] = z1; q += z1 * z1; }
                }
                quad = row16_sum(q);
                psis_row_sync();
                for (int i = c; i < Pk; i += 16) {
                    const double *Li = Lp + ev_tri(i, 0);
                    double s = 0.0;
                    for (int j = 0; j <= i; ++j) s += Li[j] * wc[j];
                    tc[i] = mv[i] + s;
                }
            }
            for (int i = Pk + c; i < Pp; i += 16) tc[i] = 0.0;
            psis_row_sync();
            // the cavity's quadratic form and the latents' prior
            double qc = 0.0, lp = 0.0;
            for (int i = c; i < d; i += 16) {
                double s = 0.0;
                for (int j = 0; j < d; ++j) s += Om[i + (size_t)j * d] * (tc[j] - mu[j]);
                qc += (tc[i] - mu[i]) * s;
            }
            for (int i = d + c; i < Pk; i += 16) lp += lap ? -fabs(tc[i]) : -0.5 * (tc[i] * tc[i]);
            qc = row16_sum(qc);
            lp = row16_sum(lp);
            if (c == 0) {
                const double lg = -0.5 * quad - sumlog - 0.5 * (double)Pk * 1.8378770664093454836;
                base[cl] = (-0.5 * qc + lp) - lg;
            }
            if (tid < 16) acc[tid] = 0.0;
            __syncthreads();
            // ---- stage B.  The rows of the site, group by group, against the slab's coefficient columns
            const bool in = c0 + col < N1;
            for (int g = 0; g < ng; ++g) {
                const PredictWg wg = a.wg[a.site_first[j0] + g];
                for (int rb = 0; rb < wg.rows; rb += EPX_PR_WG_ROWS) {
                    const int first = wg.first + rb,
                              rows = wg.rows - rb < EPX_PR_WG_ROWS ? wg.rows - rb : (int)EPX_PR_WG_ROWS;
                    const bool busy = t0 < rows;
                    RowTile t;
                    tile_load(t, a.X, D, nullptr, first, rows, t0, busy, true, y_of);
                    double ls = 0.0;
                    tile_slab(t, sl, gauss, nstep, busy, in, true,
                              [&] {
                                  if (rb != 0) return;
                                  for (int kk = tid >> 4; kk < KP; kk += 16) {
                                      double v = 0.0;
                                      if (kk <= D) v = named_value(tile_coef_elem(a.m, kk, g, ng), th + c * Pp);
                                      sl.coef[kk * 16 + c] = v;
                                  }
                                  tile_stage_scale(a.m, th + c * Pp, true, sl.lsig, sl.sig);
                              },
                              [&](int r, double f, double mu_, double ll) { if (t.row[r] >= 0) ls += ll; },
                              [&] {
                                  ls += __shfl_xor(ls, 16); ls += __shfl_xor(ls, 32);
                                  if (kq == 0) part[wave * 16 + col] = ls;
                              });
                    if (tid < 16) acc[tid] += ((part[tid] + part[16 + tid]) + part[32 + tid]) + part[48 + tid];
                }
            }
            __syncthreads();
            if (tid < 16 && c0 + tid < N1) a.terms[(size_t)j0 * 2 * N1 + (size_t)set * N1 + c0 + tid] = base[tid] + acc[tid];
            if (set == 1 && a.prop && c0 + cl < N1) {
                double *o = a.prop + ((size_t)j0 * N1 + c0 + cl) * P;
                for (int i = c; i < P; i += 16) o[i] = i < Pk ? tc[i] : 0.0;
            }
            __syncthreads();                              // the next slab overwrites the records, base and the sums
        }
    }
}
