// Tree bookkeeping, adaptation and transition control of the NUTS kernels: the part of one
// loop iteration that follows the gradient evaluation.  Textually included by every sampler kernel -- k_nuts and
// k_nuts_spec's bookkeeping wave (nuts.hip), duo_piece's state wave and its bookkeeping wave (nuts_duo.hip),
// stream_piece (nuts_stream.hip) -- so all of them run the SAME algorithm.
// Its scope is the one nuts_chain_state.inc declares (the chain's scalars with their start values: the list is at
// the top of that file); the macro it uses (EPX_INIT_DRAW) is in nuts_common.h.  The kernel itself provides:
//   the vectors, Vec<NV> or anything with the same `.v[i]`: mu-free state inv_e qs gs zq zp zg, tree ends pq pp pg mq mp mg,
//       rho psp psm, Welford sums wmean wm2, the subtree's best bq bg, and the iteration-local n_rho n_psl psr;
//   kin: kinetic energy of the state just evaluated (its log density is zlp); carry, teacher, toff; lane, wt (the wave of the chain that writes records: wt == 0), P, k, sb,
//       chain, key and the arguments `a`;
//   lambdas ld_stk(level, vector, register) / st_stk(level, vector, register, value) / flush_dh(count);
//   the macros EPX_CHAIN_EXIT (leave the chain loop), EPX_DBG_EXIT (leave after the test hook wrote the initial
//       gradient) and STAMP_LEAF.
// Optional: EPX_RESUME (bool: the chain continues an earlier piece of its run -- the initial evaluation goes
// straight to the next transition) and EPX_T_END (the transition at which this piece ends; default a.iter).
#ifndef EPX_WAVE_SUM2
#define EPX_WAVE_SUM2(a_, b_) wave_sum2(a_, b_)
#define EPX_WAVE_SUM2_DEFAULT
#endif
// The elementary functions of the bookkeeping that run once per SUBTREE (weights of the multinomial draw, Gumbel keys):
// libm's by default; a kernel whose other waves wait for this one (the row team) passes the lean ones of epx_device.h
#ifndef EPX_SM_EXP
#define EPX_SM_EXP(x) exp(x)
#define EPX_SM_LOG(x) log(x)
#define EPX_SM_LSE2(a_, b_) log_sum_exp2(a_, b_)
#define EPX_SM_MATH_DEFAULT
#endif
// The code of a finished subtree / transition is long; a kernel whose other waves wait for this one may give them a
// chance to go on at these points (the row team: nuts_duo.hip, sm_yield).  The argument is a rough count of the cycles
// of bookkeeping still ahead from that point when nothing else ends (measured on the row team's state wave, alone on its
// SIMD).  Nothing by default.
#ifndef EPX_SM_YIELD
#define EPX_SM_YIELD(cycles_ahead_) do { } while (0)
#define EPX_SM_YIELD_DEFAULT
#endif
#ifndef EPX_RESUME
#define EPX_RESUME false
#define EPX_T_END a.iter
#define EPX_PIECE_DEFAULTS
#endif
        double h = -zlp + kin;
        if (isnan(h)) h = INFINITY;

        bool do_begin_ss = false, do_ss_setup = false, do_begin_transition = false;
        bool do_begin_doubling = false, do_end_transition = false;

        if (mode == MODE_TREE) {
            // ---------------- one new leaf of the subtree being built (base_nuts::build_tree, depth 0)
            ++nleap;
            if (h - H0 > 1000.0) divergent = 1;
            const double dH = H0 - h;
            const int slot = leaf & 63;
            dhb = (lane == slot) ? dH : dhb;
            int valid = divergent ? 0 : 1;
            int l = 0;
            if (valid) {
                FORV {
                    n_rho.v[i] = zp.v[i];
                    psr.v[i] = inv_e.v[i] * zp.v[i];
                    n_psl.v[i] = psr.v[i];
                }
                // Multinomial draw inside the new subtree.  base_nuts::build_tree picks, at every merge, the
                // right half's proposal with probability w_right / (w_left + w_right); with Gumbel keys
                // (log-weight + Gumbel noise per leaf, noise from the counter-based generator) that is "the
                // half whose best key is larger, the left one on ties", so the proposal of a COMPLETED subtree
                // is its leaf with the largest key, the first one on ties -- whatever the merge order.  A
                // running best replaces the per-level copies of (proposal, gradient) that the pairwise merges
                // would carry on the stack; a subtree that fails a U-turn check is discarded as a whole.
                const double key_leaf = dH + readlane_d(gum, slot);
                if (leaf == 0 || key_leaf > b_key) {
                    b_key = key_leaf; b_plp = zlp;
                    FORV { bq.v[i] = zq.v[i]; bg.v[i] = zg.v[i]; }
                }
                int ii = leaf;
                while (ii & 1) {
                    double c1 = 0.0, c2 = 0.0;
                    FORV {
                        const bool in_p = lane + 64 * i < P;               // the vectors are 0 beyond P: not stored
                        const double Lrho = in_p ? ld_stk(l, 0, i) : 0.0;
                        const double Lpsl = in_p ? ld_stk(l, 1, i) : 0.0;
                        n_rho.v[i] += Lrho;
                        n_psl.v[i] = Lpsl;
                        c1 += psr.v[i] * n_rho.v[i];
                        c2 += n_psl.v[i] * n_rho.v[i];
                    }
                    EPX_WAVE_SUM2(c1, c2);
                    if (!(c1 > 0 && c2 > 0)) { valid = 0; break; }
                    ii >>= 1; ++l;
                }
            }
            if (valid && leaf != nleaf - 1) {
                // ---- fast path: park the node as a pending left sibling and keep integrating
                FORV {
                    if (lane + 64 * i < P) {
                        st_stk(l, 0, i, n_rho.v[i]);
                        st_stk(l, 1, i, n_psl.v[i]);
                    }
                }
                ++leaf;
                if ((leaf & 63) == 0) {
                    flush_dh(64);
                    EPX_SM_YIELD(1800);
                    double u1, u2;
                    const uint32_t li = (uint32_t)(leaf + lane);
                    rng_u2(key, (uint32_t)t + toff, K_MERGE, (uint32_t)depth, li >> 1, u1, u2);
                    gum = -EPX_SM_LOG(-EPX_SM_LOG((li & 1) ? u2 : u1));
                }
                STAMP_LEAF;
                continue;
            }
            // ---- the new subtree is complete or was rejected
            EPX_SM_YIELD(5000);
            flush_dh(slot + 1);
            if (fwd) { FORV { pq.v[i] = zq.v[i]; pp.v[i] = zp.v[i]; pg.v[i] = zg.v[i]; } plp = zlp; }
            else     { FORV { mq.v[i] = zq.v[i]; mp.v[i] = zp.v[i]; mg.v[i] = zg.v[i]; } mlp = zlp; }
            if (!valid) do_end_transition = true;
            else {
                ++depth;
                const double lw_sub = lw_m + EPX_SM_LOG(lw_s);
                bool take;
                if (lw_sub > lsw) take = true;
                else take = readlane_d(u_dir, 16 + depth - 1) < EPX_SM_EXP(lw_sub - lsw);
                if (take) { FORV { qs.v[i] = bq.v[i]; gs.v[i] = bg.v[i]; } lps = b_plp; }
                lsw = EPX_SM_LSE2(lsw, lw_sub);
                double c1 = 0.0, c2 = 0.0;
                FORV {
                    rho.v[i] += n_rho.v[i];
                    if (fwd) psp.v[i] = psr.v[i]; else psm.v[i] = psr.v[i];
                    c1 += psp.v[i] * rho.v[i];
                    c2 += psm.v[i] * rho.v[i];
                }
                EPX_WAVE_SUM2(c1, c2);
                if (!(c1 > 0 && c2 > 0)) do_end_transition = true;
                else if (depth >= a.max_depth) do_end_transition = true;
                else do_begin_doubling = true;
            }
        } else if (mode == MODE_INIT) {
            FORV { gs.v[i] = zg.v[i]; }
            lps = zlp;
            int fin = isfinite(zlp) ? 1 : 0;
            FORV { if (!isfinite(zg.v[i])) fin = 0; }
            fin = __all(fin);
            if (a.dbg) {
                if (wt == 0) {
                    if (lane == 0) a.dbg[0] = zlp;
                    FORV { const int e = lane + 64 * i; if (e < a.P) a.dbg[1 + e] = zg.v[i]; }
                }
                EPX_DBG_EXIT;
            }
            if (!fin && a.init_mode == 0 && !teacher && !EPX_RESUME && init_try < 99) {
                // init = 'random': Stan draws the start again, up to 100 times, until log density and gradient are finite
                // (stan::services::util::initialize behind PyStan's sampling(), /root/reference/epstan/util.py:716);
                // a given start -- zeros, the previous draws -- gets one attempt.
                ++init_try;
                FORV {
                    const int e = lane + 64 * i;
                    double q0 = 0.0;
                    if (e < P) EPX_INIT_DRAW(q0, e, init_try)
                    qs.v[i] = q0; zq.v[i] = q0; zp.v[i] = 0.0; zg.v[i] = 0.0;
                }
                eps_l = 0.0;                            // (the next "leapfrog" is the evaluation at the new start)
            } else {
                if (!fin) { failed = 1; EPX_CHAIN_EXIT; }
                ss_t = 0; ss_after_update = 0;
                if (teacher || EPX_RESUME) do_begin_transition = true; else do_begin_ss = true;
            }
        } else {
            const double dH = H0 - h;
            bool done = false;
            if (ss_trial == 0) ss_dir = dH > LOG08 ? 1 : -1;
            else {
                if (ss_dir == 1 && !(dH > LOG08)) done = true;
                else if (ss_dir == -1 && !(dH < LOG08)) done = true;
                else eps = ss_dir == 1 ? 2.0 * eps : 0.5 * eps;
                if (!done && (eps > 1e7 || eps == 0.0)) done = true;
                if (!done && ss_trial > 200) done = true;
            }
            if (done) {
                if (ss_after_update) { da_mu = log(10.0 * eps); da_count = 0; s_bar = 0; x_bar = 0; }
                do_begin_transition = true;
            } else { ++ss_trial; do_ss_setup = true; }
        }

        if (do_end_transition) {
            EPX_SM_YIELD(12000);
            const double accept = sum_metro / (double)nleap;
            const double eps_used = eps;
            eps_sum += eps;
            nleap_tot += nleap;
            bool metric_updated = false;
            if (t < a.warmup) {
                // stepsize_adaptation::learn_stepsize
                da_count += 1.0;
                const double as = accept > 1.0 ? 1.0 : accept;
                const double eta_da = 1.0 / (da_count + T0);
                s_bar = (1.0 - eta_da) * s_bar + eta_da * (DELTA - as);
                const double x = da_mu - s_bar * sqrt(da_count) / GAMMA;
                const double x_eta = exp(-KAPPA * log(da_count));          // da_count^(-kappa)
                x_bar = (1.0 - x_eta) * x_bar + x_eta * x;
                eps = exp(x);
                // var_adaptation::learn_variance
                // (carried adaptation keeps the metric it started with: step size only)
                const bool in_win = !carry && (va_counter >= va_init_buf) && (va_counter < a.warmup - va_term) &&
                                    (va_counter != a.warmup);
                if (in_win) {
                    va_n += 1.0;
                    FORV {
                        const double delta = qs.v[i] - wmean.v[i];
                        wmean.v[i] += delta / va_n;
                        wm2.v[i] += (qs.v[i] - wmean.v[i]) * delta;
                    }
                }
                const bool end_win = !carry && (va_counter == va_next) && (va_counter != a.warmup);
                if (end_win) {
                    if (va_next != a.warmup - va_term - 1) {
                        va_wsize *= 2;
                        va_next = va_counter + va_wsize;
                        if (va_next != a.warmup - va_term - 1) {
                            const int boundary = va_next + 2 * va_wsize;
                            if (boundary >= a.warmup - va_term) va_next = a.warmup - va_term - 1;
                        }
                    }
                    FORV {
                        const double s2 = va_n > 1.0 ? wm2.v[i] / (va_n - 1.0) : 0.0;
                        inv_e.v[i] = (va_n / (va_n + 5.0)) * s2 + 1e-3 * (5.0 / (va_n + 5.0));
                        wmean.v[i] = 0.0; wm2.v[i] = 0.0;
                    }
                    va_n = 0;
                    metric_updated = true;
                }
                ++va_counter;
                if (t == a.warmup - 1 && !metric_updated) eps = exp(x_bar);     // complete_adaptation
            } else {
                acc_sum += accept; depth_sum += depth; ndiv += divergent; ++npost;
                if ((t - a.warmup) % a.thin == 0) {
                    if (wt == 0) {
                        // records are a.P wide (a.P > P only for multi-group sites; vectors are 0 beyond P)
                        double *dst = a.draws + (((size_t)k * a.chains + chain) * a.nkeep + kept) * a.P;
                        FORV { const int e = lane + 64 * i; if (e < a.P) __builtin_nontemporal_store((double)qs.v[i], dst + e); }     // (written once, read by the host side)
                    }
                    ++kept;
                }
            }
            if (a.trace && sb < a.trace_sites && wt == 0) {
                // test hook (epx_set_trace): one record per transition, warm-up included -- step size used, leapfrogs, accept
                // statistic, depth, divergent, the step size after learn_stepsize / complete_adaptation (in front of the search
                // that follows a new metric), the sum of the metric after learn_variance, log density, the new sample
                double *tr = a.trace + (((size_t)sb * a.chains + chain) * a.iter + t) * (size_t)(8 + a.P);
                double ms_ = 0.0;
                FORV { if (lane + 64 * i < P) ms_ += inv_e.v[i]; }
                ms_ = wave_sum(ms_);
                if (lane == 0) {
                    tr[0] = eps_used; tr[1] = (double)nleap; tr[2] = accept; tr[3] = (double)depth; tr[4] = (double)divergent;
                    tr[5] = eps; tr[6] = ms_; tr[7] = lps;
                }
                FORV { const int e = lane + 64 * i; if (e < a.P) tr[8 + e] = qs.v[i]; }
            }
            ++t;
            if (metric_updated) { ss_t = (uint32_t)t; ss_after_update = 1; do_begin_ss = true; }
            else do_begin_transition = true;
        }

        if (do_begin_ss) {
            if (eps == 0.0 || eps > 1e7 || isnan(eps)) {
                if (ss_after_update) { da_mu = log(10.0 * eps); da_count = 0; s_bar = 0; x_bar = 0; }
                do_begin_ss = false; do_begin_transition = true;
            }
            else { ss_trial = 0; ss_dir = 0; do_ss_setup = true; mode = MODE_SS; }
        }
        if (do_ss_setup) {
            double s = 0.0;
            FORV {
                const int e = lane + 64 * i;
                zp.v[i] = e < P ? rng_normal(key, ss_t, K_SSMOM, e, (uint32_t)ss_trial) / sqrt(inv_e.v[i]) : 0.0;
                zq.v[i] = qs.v[i]; zg.v[i] = gs.v[i];
                s += inv_e.v[i] * zp.v[i] * zp.v[i];
            }
            H0 = -lps + 0.5 * wave_sum(s);
            eps_l = eps;
        }
        if (do_begin_transition) {
            if (t >= EPX_T_END) { EPX_CHAIN_EXIT; }
            EPX_SM_YIELD(6000);
            double s = 0.0;
            FORV {
                const int e = lane + 64 * i;
                pp.v[i] = e < P ? rng_normal(key, (uint32_t)t + toff, K_MOM, e, 0) / sqrt(inv_e.v[i]) : 0.0;
                pq.v[i] = qs.v[i]; pg.v[i] = gs.v[i];
                mq.v[i] = qs.v[i]; mg.v[i] = gs.v[i]; mp.v[i] = pp.v[i];
                psp.v[i] = inv_e.v[i] * pp.v[i]; psm.v[i] = psp.v[i];
                rho.v[i] = pp.v[i];
                s += inv_e.v[i] * pp.v[i] * pp.v[i];
            }
            plp = lps; mlp = lps;
            H0 = -lps + 0.5 * wave_sum(s);
            lsw = 0.0; sum_metro = 0.0; depth = 0; nleap = 0; divergent = 0;
            // direction / top-level uniforms of this transition in one Philox batch
            u_dir = rng_uniform(key, (uint32_t)t + toff, lane < 16 ? K_DIR : K_TOP, (uint32_t)(lane & 15), 0);
            mode = MODE_TREE;
            do_begin_doubling = true;
        }
        if (do_begin_doubling) {
            EPX_SM_YIELD(2500);
            fwd = readlane_d(u_dir, depth) > 0.5 ? 1 : 0;
            eps_l = fwd ? eps : -eps;
            if (fwd) { FORV { zq.v[i] = pq.v[i]; zp.v[i] = pp.v[i]; zg.v[i] = pg.v[i]; } zlp = plp; }
            else     { FORV { zq.v[i] = mq.v[i]; zp.v[i] = mp.v[i]; zg.v[i] = mg.v[i]; } zlp = mlp; }
            leaf = 0; nleaf = 1 << depth;
            lw_m = -INFINITY; lw_s = 0.0;
            EPX_SM_YIELD(1800);
            {
                double u1, u2;
                rng_u2(key, (uint32_t)t + toff, K_MERGE, (uint32_t)depth, (uint32_t)(lane >> 1), u1, u2);
                gum = -EPX_SM_LOG(-EPX_SM_LOG((lane & 1) ? u2 : u1));
            }
        }
#ifdef EPX_WAVE_SUM2_DEFAULT
#undef EPX_WAVE_SUM2
#undef EPX_WAVE_SUM2_DEFAULT
#endif
#ifdef EPX_SM_MATH_DEFAULT
#undef EPX_SM_EXP
#undef EPX_SM_LOG
#undef EPX_SM_LSE2
#undef EPX_SM_MATH_DEFAULT
#endif
#ifdef EPX_SM_YIELD_DEFAULT
#undef EPX_SM_YIELD
#undef EPX_SM_YIELD_DEFAULT
#endif
#ifdef EPX_PIECE_DEFAULTS
#undef EPX_RESUME
#undef EPX_T_END
#undef EPX_PIECE_DEFAULTS
#endif
