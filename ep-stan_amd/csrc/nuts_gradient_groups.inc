// One leapfrog + gradient evaluation for a site that holds SEVERAL groups of the hierarchical
// model (K < J: experiment/models/m{1..5}b.stan, theta = [phi (d) | eta (ng) | etb (ng x D)]) on the
// one-workgroup-per-chain layout: textually included by k_nuts_spec<..., GRP = true> in place of
// nuts_gradient.inc.  The four gradient waves share the work by GROUP: wave w takes groups
// w, w + 4, ... (a group's rows are contiguous; its own alpha_g, beta_g are wave-uniform, so the
// row pass is the single-group one), every wave takes its share of the columns of the Omega
// mat-vec, and after the ONE barrier of the leapfrog every wave assembles the whole gradient from
// the per-group records in LDS (identical instructions on identical inputs in all four waves).
// Expects in scope what nuts_gradient.inc expects, plus ng (groups of this site), gl_s (LDS, ng + 1
// row limits relative to the site), qcopy (LDS, 4 x 2 x 64 NV doubles: per-wave copies of q and exp(q)) and
// GREC / WREC, the record sizes; defines kin and sets zlp (or lp_lane / ll_u with EPX_DEFER_ENERGY).
        double kin = 0.0;
        FORV zp.v[i] += 0.5 * eps_l * zg.v[i];
        FORV zq.v[i] += eps_l * inv_e.v[i] * zp.v[i];
        {
            V eq;
            FORV eq.v[i] = exp_d(zq.v[i]);
            // q and exp(q) also go to a wave-private LDS copy: every "element e of the vector" below is then
            // one LDS read instead of a lane exchange per register (and may sit in divergent code)
            double *qc = qcopy + (size_t)wt * 2 * 64 * NV, *eqc = qc + 64 * NV;
            FORV { qc[64 * i + lane] = zq.v[i]; eqc[64 * i + lane] = eq.v[i]; }
            constexpr int O = GAUSS ? 1 : 0;                // Gaussian likelihood: phi = [log sigma | the b-model's phi]
            const int isa = (model >= 3 ? 1 : 0) + O;       // element of log sigma_a
            const double sa = elemU(eq, isa);
            const double a0 = model >= 3 ? elemU(zq, O) : 0.0;
            const double inv_s2 = GAUSS ? exp_d(-2.0 * elemU(zq, 0)) : 0.0;
            (void)inv_s2;
            double *wrec = xch + (size_t)parity * nuts_group_exchange(NV, WPC, a.ngmax);       // per-wave records
            double *grec = wrec + WPC * WREC;                                          // per-group records
            STAMP(0);
            // ---- likelihood, group by group: f = alpha_g + x.beta_g, res = y - sigmoid(f), acc += res x
            double ll = 0.0, wprod = 1.0;
            for (int g = wt; g < ng; g += WPC) {
                const double eta_g = elemU(zq, d + g);
                const double alpha = a0 + eta_g * sa;
                double beta_l = 0.0;
                if (lane < D) {
                    const double etb = model == 0 ? 0.0 : qc[d + ng + g * D + lane];
                    if (model == 0) beta_l = qc[O + 1 + lane];
                    else if (model == 1) beta_l = etb * eqc[O + 1];
                    else if (model == 2) beta_l = etb * eqc[O + 1 + lane];
                    else beta_l = qc[O + 2 + lane] + etb * eqc[O + 2 + D + lane];
                }
                double bs[DP];
#pragma unroll
                for (int j = 0; j < DP; ++j) bs[j] = readlane_d(beta_l, j);
                double acc[DP];
#pragma unroll
                for (int j = 0; j < DP; ++j) acc[j] = 0.0;
                double da = 0.0;
                const int r_hi = gl_s[g + 1];
                for (int r = gl_s[g] + lane; r < r_hi; r += 64) {
                    const double2 *rowp = reinterpret_cast<const double2 *>(Xs + (size_t)r * DP);
                    const int sw = (r / RPL) & (SPR - 1);
                    double x[DP];
#pragma unroll
                    for (int jp = 0; jp < SPR; ++jp) {
                        const double2 v = rowp[jp ^ sw];
                        x[2 * jp] = v.x; x[2 * jp + 1] = v.y;
                    }
                    double f0 = alpha, f1 = 0.0;
#pragma unroll
                    for (int j = 0; j < DP; j += 2) { f0 = fma(x[j], bs[j], f0); f1 = fma(x[j + 1], bs[j + 1], f1); }
                    double l, w, res;
                    if constexpr (GAUSS) {      // y ~ normal(f, sigma)
                        const double rr = y_at(r) - (f0 + f1);
                        res = rr * inv_s2; l = -0.5 * rr * res; w = 1.0;
                    } else logistic_split(f0 + f1, (double)ys[r], l, w, res);
                    ll += l; wprod *= w; da += res;
#pragma unroll
                    for (int j = 0; j < DP; ++j) acc[j] = fma(res, x[j], acc[j]);
                }
                butterfly<DP, 5>(acc, lane);                // lane ends with the sum of acc[lane >> (6 - LOG)]
                da = wave_sum(da);
                grec[(size_t)g * GREC + lane] = acc[0];
                if (lane == 0) grec[(size_t)g * GREC + 64] = da;
            }
            if constexpr (!GAUSS) ll -= log_ge1_d(wprod);
            ll = wave_sum(ll);
            STAMP(1);
            STAMP(2);
            // ---- cavity term: this wave's share of the columns of Ov = Omega (phi - mu)
            V vv, Ov;
            int ec[NV];
            FORV { const int e = lane + 64 * i; vv.v[i] = e < d ? zq.v[i] - mu.v[i] : 0.0; Ov.v[i] = 0.0; ec[i] = e < d ? e : d - 1; }
            {
                const int jb = (wt * d) / WPC, je = ((wt + 1) * d) / WPC;
#pragma unroll
                for (int ii = 0; ii < NV; ++ii) {
                    const int lo = jb > 64 * ii ? jb : 64 * ii;
                    const int hi = je < 64 * (ii + 1) ? je : 64 * (ii + 1);
                    constexpr int CU = 2;
                    for (int j = lo; j < hi; j += CU) {
                        double vj[CU], cc[CU][NV];
#pragma unroll
                        for (int u = 0; u < CU; ++u) {
                            const bool ok = j + u < hi;
                            const int ju = ok ? j + u : j;
                            const double t2 = readlane_d(vv.v[ii], ju & 63);
                            vj[u] = ok ? t2 : 0.0;
                            FORV cc[u][i] = om_at(ju * d + ec[i]);
                        }
#pragma unroll
                        for (int u = 0; u < CU; ++u) { FORV Ov.v[i] = fma(cc[u][i], vj[u], Ov.v[i]); }
                    }
                }
            }
            STAMP(3);
            {
                double *rec = wrec + (size_t)wt * WREC;
                FORV rec[64 * i + lane] = Ov.v[i];
                if (lane == 0) rec[64 * NV] = ll;
                __syncthreads();
                EPX_AFTER_EXCHANGE_BARRIER;
                ll = 0.0;
                FORV Ov.v[i] = 0.0;
#pragma unroll
                for (int w = 0; w < WPC; ++w) {
                    const double *rw = wrec + (size_t)w * WREC;
                    FORV Ov.v[i] += rw[64 * i + lane];
                    ll += rw[64 * NV];
                }
                parity ^= 1;
            }
            STAMP(4);
            ll = uniform_d(ll);
            // Gaussian likelihood: d/d(log sigma) = sum (y-f)^2 / sigma^2 - n = -2 ll - n, and lp gets -n log sigma
            double c_ls = 0.0;
            if constexpr (GAUSS) { c_ls = -2.0 * ll - (double)n; ll -= (double)n * elemU(zq, 0); }
            (void)c_ls;
            // ---- chain rule back to (phi, eta_g, etb_g); G_g[c] = sum over the rows of group g of res x[c]
            auto Gg = [&](int g, int c) { return grec[(size_t)g * GREC + ((c << (6 - LOG)) & 63)]; };
            auto dag = [&](int g) { return grec[(size_t)g * GREC + 64]; };
            double dot = 0.0;
            if (model == 1) {           // m2b: d log sigma_b = sb * sum_g sum_c G_g[c] etb_g[c]
                double tsum = 0.0;
                FORV {
                    const int e = lane + 64 * i;
                    if (e >= d + ng && e < P) {
                        const int idx = e - d - ng;
                        int gg = 0;
                        for (int t = 1; t < ng; ++t) gg += idx >= t * D ? 1 : 0;
                        tsum += Gg(gg, idx - gg * D) * zq.v[i];
                    }
                }
                dot = wave_sum(tsum);
            }
            double s_da = 0.0, s_daeta = 0.0;
            for (int g0 = 0; g0 < ng; g0 += 4) {
                double t[4], e4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int g = g0 + u < ng ? g0 + u : ng - 1; t[u] = dag(g); e4[u] = qc[d + g]; }
#pragma unroll
                for (int u = 0; u < 4; ++u) { if (g0 + u < ng) { s_da += t[u]; s_daeta += t[u] * e4[u]; } }
            }
            double lpt = 0.0;
            FORV {
                const int e = lane + 64 * i;
                const double q = zq.v[i];
                const bool in_phi = e < d, in_par = e < P;
                const double ov = in_phi ? Ov.v[i] : 0.0;
                lpt += in_phi ? -0.5 * vv.v[i] * ov : (in_par ? (laplace ? -fabs(q) : -0.5 * q * q) : 0.0);
                const double pr = laplace ? (double)((q > 0) - (q < 0)) : q;
                double g = 0.0;
                if (in_phi) {
                    // hyper-parameters: every group contributes
                    double add = 0.0;
                    const int eb = e - O;                   // index in the b-model's phi
                    if (GAUSS && e == 0) add = c_ls;
                    else if (model >= 3 && eb == 0) add = s_da;
                    else if (e == isa) add = s_daeta * sa;
                    else if (model == 1) add = eb == 1 ? dot * eqc[O + 1] : 0.0;
                    else {
                        // slope blocks: m1b beta (1..D); m3b log sigma_b (1..D); m4b/m5b mu_b (2..1+D), log sigma_b (2+D..)
                        const int c = model >= 3 ? (eb < 2 + D ? eb - 2 : eb - 2 - D) : eb - 1;
                        const bool scale = model == 2 || (model >= 3 && eb >= 2 + D);
                        // four groups per round: their (independent) LDS reads are in flight together
                        for (int g0 = 0; g0 < ng; g0 += 4) {
                            double Gv[4], et[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const int gg = g0 + u < ng ? g0 + u : ng - 1;
                                Gv[u] = Gg(gg, c);
                                et[u] = scale ? qc[d + ng + gg * D + c] : 1.0;
                            }
#pragma unroll
                            for (int u = 0; u < 4; ++u) add += g0 + u < ng ? Gv[u] * et[u] : 0.0;
                        }
                        add = scale ? add * eq.v[i] : add;
                    }
                    g = add - ov;
                } else if (e < d + ng) {
                    g = dag(e - d) * sa - pr;                               // eta_g
                } else if (in_par) {
                    const int idx = e - d - ng;                             // etb_g[c]: g = idx / D without the division
                    int gg = 0;
                    for (int t = 1; t < ng; ++t) gg += idx >= t * D ? 1 : 0;
                    const int c = idx - gg * D;
                    const double sbv = model == 1 ? eqc[O + 1] : eqc[O + (model == 2 ? 1 : 2 + D) + c];
                    g = Gg(gg, c) * sbv - pr;
                }
                zg.v[i] = in_par ? g : 0.0;
            }
            double ks = 0.0;
            FORV { zp.v[i] += 0.5 * eps_l * zg.v[i]; ks += inv_e.v[i] * zp.v[i] * zp.v[i]; }
#if EPX_DEFER_ENERGY
            lp_lane = lpt; ll_u = ll; (void)ks;
#else
            wave_sum2(lpt, ks);
            zlp = lpt + ll;
            kin = 0.5 * ks;
#endif
        }
