// Pareto-smoothed importance sampling of ONE row's leave-one-out ratios (include/epx.h, enum epx_loo, states the
// definition; loo.psis_host is the NumPy statement): from the S log-likelihoods ll_s of a row under the draws of its site
// to ELPD, KHAT and WESS.  Used by k_loo and k_psis_rows (predict.hip): psis_row = psis_smooth (the order, the fit, the
// smoothed tail and the normaliser) + the reductions.  k_reweight (dense.hip) calls psis_smooth alone on the log ratios of
// two cavities and forms every draw's own weight from what it leaves.
//
// A row is worked on by the 16 lanes of one DPP row (lane c = lane & 15 takes the draws s = c, c + 16, ...), all of them
// active, every argument the same in the 16 lanes; four rows share a wave.  Every sum is a lane's own terms in
// increasing s followed by the four fixed DPP steps of row16_sum: no atomics, the same bits on every call, whatever
// else runs.  The log-likelihoods are only read:
//   - the ORDER.  Only the last M of the order by (lr_s, s) and the value in front of them are needed, M <= 3 sqrt(S) + 1,
//     so nothing is sorted.  A bisection over the bit pattern of a threshold T (each step one counting pass of the row)
//     finds between M + 1 and M + 17 CANDIDATES |lr| < T, which hold the tail and u; the lanes append theirs to a list
//     in the row's scratch, and every candidate counts the candidates that come behind it (every lane of the row reads
//     the same entry: a broadcast): C^2 instead of S^2 comparisons.  A candidate with rank < M from the top writes its ll
//     into the row's tail array at its rank, the one of rank M is `u`; the order is total, so every slot has exactly
//     one writer.  When ties keep the bisection from landing (a constant row, a few levels) every draw is counted
//     against every draw instead: the same ranks, S^2 comparisons.
//   - the FIT.  The m = 30 + floor(sqrt(M)) candidates b_i are dealt to the lanes; a lane walks all M excesses for its
//     candidates (a broadcast read each), the profile log-likelihoods L_i meet in the row's scratch, and the weights
//     w_i = 1 / sum_j exp(L_j - L_i) are formed as written.  The library's log1p / log / expm1 / exp here (a few thousand
//     per row): the excesses x_j are differences of nearby exponentials and the fit is ill-conditioned in them.
//   - the REDUCTIONS.  A draw belongs to the tail exactly when (lr_s, s) > (lr_u, u): the sums over the draws in front
//     of the tail take ll from the tile, those over the tail take the smoothed values from the scratch.  The second
//     log-sum-exp is taken about max(e_u, max_tail e_j), e = lw + ll, which is the largest term up to the rounding of
//     lr + ll (in front of the tail lr_s + ll_s = -max(-ll) but for rounding).
#pragma once
#include "epx_device.h"

namespace epx {

enum { PSIS_MIN_TAIL = 5, PSIS_FIT_MAX = 64 };

// M = min(floor(S / 5), ceil(3 sqrt(S))) in integers
__host__ __device__ inline int psis_tail_length(int S) {
    long long c = 0;
    while (c * c < 9LL * S) ++c;
    const long long f = S / 5;
    return (int)(f < c ? f : c);
}
// m = 30 + floor(sqrt(M))
__host__ __device__ inline int psis_fit_points(int M) {
    int r = 0;
    while ((long long)(r + 1) * (r + 1) <= M) ++r;
    return 30 + r;
}
// doubles of scratch per row: [tail ll (Mp) | candidates' lr, then tail x, then the smoothed lr (Cp) | candidates' draw
// indices (Cp ints) | L_i (PSIS_FIT_MAX; first the lanes' candidate counts) | ll_u, u]
__host__ __device__ inline int psis_tail_pad(int M) { return (M + 1) / 2 * 2; }
__host__ __device__ inline int psis_cand_cap(int M) { return psis_tail_pad(M) + 16; }      // candidates the list holds
__host__ __device__ inline int psis_scratch_doubles(int M) {
    return psis_tail_pad(M) + psis_cand_cap(M) + psis_cand_cap(M) / 2 + PSIS_FIT_MAX + 2;
}

// all 16 lanes of a DPP row end with the row's sum / maximum
__device__ inline double row16_sum(double v) {
    v += dpp_d<DPP_QUAD_XOR1>(v);
    v += dpp_d<DPP_QUAD_XOR2>(v);
    v += dpp_d<DPP_ROW_HALF_MIRROR>(v);
    v += dpp_d<DPP_ROW_MIRROR>(v);
    return v;
}
__device__ inline double row16_max(double v) {
    v = fmax(v, dpp_d<DPP_QUAD_XOR1>(v));
    v = fmax(v, dpp_d<DPP_QUAD_XOR2>(v));
    v = fmax(v, dpp_d<DPP_ROW_HALF_MIRROR>(v));
    v = fmax(v, dpp_d<DPP_ROW_MIRROR>(v));
    return v;
}

// what the 16 lanes of a row wrote to the row's scratch is read by the others behind this (they share a wave: LDS
// operations of a wave complete in order; the fences keep the compiler from moving them)
__device__ inline void psis_row_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// 1 if every ll_s of the row is finite (all 16 lanes get the answer)
__device__ inline bool psis_row_finite(const double *ll, int S, int c) {
    double bad = 0.0;
    for (int s = c; s < S; s += 16) bad += isfinite(ll[s]) ? 0.0 : 1.0;
    return row16_sum(bad) == 0.0;
}

struct PsisOut { double elpd, khat, wess; };

// What the smoothing (steps 1-7) leaves for whoever forms sums over the smoothed weights: draw s lies in the tail exactly
// when smoothed and (lr_s, s) > (u_lr, u_at), lr_s = -ll_s - mx; the tail's smoothed lr, ascending, are then in the row's
// scratch at scr + psis_tail_pad(M) and its ll at scr; lw = lr - lse.
struct PsisFit { double mx, khat, u_lr, u_ll, lse; int u_at; bool smoothed; };

// ll: the row's S FINITE log-likelihoods (LDS or global); M, mfit: psis_tail_length(S), psis_fit_points(M); scr: the row's
// psis_scratch_doubles(M) doubles of LDS; tail_s: NULL, or M ints of LDS that get the draw index of every tail member in
// rank order (k_reweight, dense.hip: it needs every draw's own weight)
__device__ inline PsisFit psis_smooth(const double *ll, int S, int M, int mfit, double *scr, int c, int *tail_s) {
    const int Mp = psis_tail_pad(M), Cp = psis_cand_cap(M);
    double *tail_ll = scr, *tail_x = scr + Mp, *cand_v = tail_x;
    int *cand_s = reinterpret_cast<int *>(scr + Mp + Cp);
    double *fitL = scr + Mp + Cp + Cp / 2, *uslot = fitL + PSIS_FIT_MAX;
    // 1. lr_s = -ll_s - max(-ll): the largest is 0
    double mx = -INFINITY;
    for (int s = c; s < S; s += 16) mx = fmax(mx, -ll[s]);
    mx = row16_max(mx);

    PsisFit o;
    o.khat = INFINITY;
    bool smoothed = false;
    double u_lr = INFINITY, u_ll = -mx;                   // not smoothed: nothing lies behind u; lr = 0 stands for the rest
    int u_at = 0;
    if (M >= PSIS_MIN_TAIL) {
        // 3. the last M of the order by (lr, s), and the value in front of them.  First a threshold T with between M + 1
        // and `cap` draws at |lr| < T, by bisection over the bit pattern of T (at most 63 steps whatever the scale of lr)
        const int cap = psis_cand_cap(M);
        double T = INFINITY;
        int C = S, mine = (S - c + 15) / 16;
        bool listed = S <= cap;
        if (!listed) {
            unsigned long long lo = 0, hi = 0x7ff0000000000000ull;        // fewer than M + 1 below lo, more than cap below hi
            while (hi - lo > 1) {
                const unsigned long long mid = lo + (hi - lo) / 2;
                const double Tm = __longlong_as_double((long long)mid);
                int n = 0;
                for (int s = c; s < S; s += 16) n += -(-ll[s] - mx) < Tm;
                const int count = (int)row16_sum((double)n);
                if (count < M + 1) lo = mid;
                else if (count > cap) hi = mid;
                else { listed = true; T = Tm; C = count; mine = n; break; }
            }
        }
        if (listed) {
            // the C candidates (lr, s), in any order: a lane appends its own behind those of the lanes in front of it
            fitL[c] = (double)mine;
            psis_row_sync();
            int at = 0;
            for (int l = 0; l < c; ++l) at += (int)fitL[l];
            for (int s = c; s < S; s += 16) {
                const double lr = -ll[s] - mx;
                if (-lr < T) { cand_v[at] = lr; cand_s[at] = s; ++at; }
            }
            psis_row_sync();
            for (int base = 0; base < C; base += 64) {
                double v[4];
                int si[4], cnt[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int p = base + c + 16 * i;
                    v[i] = p < C ? cand_v[p] : 0.0;
                    si[i] = p < C ? cand_s[p] : 0;
                    cnt[i] = p < C ? 0 : M + 1;
                }
#pragma unroll 4
                for (int t = 0; t < C; ++t) {
                    const double vt = cand_v[t];
                    const int st = cand_s[t];
#pragma unroll
                    for (int i = 0; i < 4; ++i) cnt[i] += (vt > v[i]) | ((vt == v[i]) & (st > si[i]));
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (cnt[i] < M) {
                        tail_ll[M - 1 - cnt[i]] = ll[si[i]];
                        if (tail_s) tail_s[M - 1 - cnt[i]] = si[i];
                    } else if (cnt[i] == M) { uslot[0] = ll[si[i]]; uslot[1] = (double)si[i]; }
                }
            }
        } else {
            // ties across the threshold (a constant row, a few levels): every draw against every draw
            for (int base = 0; base < S; base += 64) {
                const int s0 = base + c;
                double v[4];
                int si[4], cnt[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    si[i] = s0 + 16 * i;
                    v[i] = si[i] < S ? -ll[si[i]] - mx : 0.0;
                    cnt[i] = si[i] < S ? 0 : M + 1;
                }
                for (int t = 0; t < S; ++t) {
                    const double vt = -ll[t] - mx;
#pragma unroll
                    for (int i = 0; i < 4; ++i) cnt[i] += (vt > v[i]) | ((vt == v[i]) & (t > si[i]));
                    if ((t & 31) == 31) {                                 // (all of them out of the tail: on to the next four)
                        const bool alive = (cnt[0] <= M) | (cnt[1] <= M) | (cnt[2] <= M) | (cnt[3] <= M);
                        if (__builtin_amdgcn_ballot_w64(alive) == 0) break;
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (cnt[i] < M) {
                        tail_ll[M - 1 - cnt[i]] = ll[si[i]];
                        if (tail_s) tail_s[M - 1 - cnt[i]] = si[i];
                    } else if (cnt[i] == M) { uslot[0] = ll[si[i]]; uslot[1] = (double)si[i]; }
                }
            }
        }
        psis_row_sync();
        const double ull = uslot[0];
        const int uat = (int)uslot[1];
        const double ulr = -ull - mx, eu = exp(ulr);
        // 4. the excesses, ascending
        for (int j = c; j < M; j += 16) tail_x[j] = exp(-tail_ll[j] - mx) - eu;
        psis_row_sync();
        const int q = (int)floor(M / 4.0 + 0.5);
        const double xq = tail_x[q - 1], xM = tail_x[M - 1];
        if (xq > 0.0 && xM > xq) {
            // 5. Zhang & Stephens
            const double dM = (double)M;
            double bpart = 0.0;
            for (int i = c + 1; i <= mfit; i += 16) {
                const double b = 1.0 / xM + (1.0 - sqrt((double)mfit / ((double)i - 0.5))) / (3.0 * xq);
                double ks = 0.0;
                for (int j = 0; j < M; ++j) ks += log1p(-b * tail_x[j]);
                const double k = ks / dM;
                fitL[i - 1] = dM * (log(-b / k) - k - 1.0);
            }
            psis_row_sync();
            for (int i = c + 1; i <= mfit; i += 16) {
                const double b = 1.0 / xM + (1.0 - sqrt((double)mfit / ((double)i - 0.5))) / (3.0 * xq);
                const double Li = fitL[i - 1];
                double den = 0.0;
                for (int j = 0; j < mfit; ++j) den += exp(fitL[j] - Li);
                bpart += b * (1.0 / den);
            }
            const double b = row16_sum(bpart);
            double ks = 0.0;
            for (int j = c; j < M; j += 16) ks += log1p(-b * tail_x[j]);
            const double k = row16_sum(ks) / dM;
            const double sigma = -k / b;
            const double khat = (dM * k + 5.0) / (dM + 10.0);
            if (isfinite(khat)) {
                // 6. the tail's ratios in rank order become the fitted distribution's quantiles (NaN stays NaN)
                psis_row_sync();
                for (int j = c; j < M; j += 16) {
                    const double l1 = log1p(-((double)j + 0.5) / dM);
                    const double qj = khat == 0.0 ? -sigma * l1 : (sigma / khat) * expm1(-khat * l1);
                    const double nl = log(eu + qj);
                    tail_x[j] = nl > 0.0 ? 0.0 : nl;
                }
                psis_row_sync();
                smoothed = true;
                o.khat = khat;
                u_lr = ulr; u_ll = ull; u_at = uat;
            }
        }
    }
    // 7. lw = lr - logsumexp(lr)
    double top = smoothed ? u_lr : 0.0;
    if (smoothed) {
        double tm = -INFINITY;
        for (int j = c; j < M; j += 16) tm = fmax(tm, tail_x[j]);     // (a NaN loses here and shows in the sums)
        top = fmax(top, row16_max(tm));
    }
    double s1 = 0.0;
    for (int s = c; s < S; s += 16) {
        const double lr = -ll[s] - mx;
        const bool in_tail = (lr > u_lr) | ((lr == u_lr) & (s > u_at));
        if (!in_tail) s1 += exp_d(lr - top);
    }
    if (smoothed)
        for (int j = c; j < M; j += 16) s1 += exp_d(tail_x[j] - top);
    o.lse = top + log(row16_sum(s1));
    o.mx = mx; o.u_lr = u_lr; o.u_ll = u_ll; o.u_at = u_at; o.smoothed = smoothed;
    return o;
}

__device__ inline PsisOut psis_row(const double *ll, int S, int M, int mfit, double *scr, int c) {
    const PsisFit f = psis_smooth(ll, S, M, mfit, scr, c, nullptr);
    const int Mp = psis_tail_pad(M);
    const double *tail_ll = scr, *tail_x = scr + Mp;
    const double mx = f.mx, u_lr = f.u_lr, u_ll = f.u_ll, lse = f.lse;
    const int u_at = f.u_at;
    const bool smoothed = f.smoothed;
    PsisOut o;
    o.khat = f.khat;
    // 8., 9. ELPD = logsumexp(lw + ll), WESS = 1 / sum exp(2 lw)
    double me = ((smoothed ? u_lr : 0.0) - lse) + u_ll;
    if (smoothed) {
        double tm = -INFINITY;
        for (int j = c; j < M; j += 16) tm = fmax(tm, (tail_x[j] - lse) + tail_ll[j]);
        me = fmax(me, row16_max(tm));
    }
    double s2 = 0.0, s3 = 0.0;
    for (int s = c; s < S; s += 16) {
        const double l = ll[s], lr = -l - mx;
        const bool in_tail = (lr > u_lr) | ((lr == u_lr) & (s > u_at));
        if (!in_tail) {
            const double lw = lr - lse;
            s2 += exp_d((lw + l) - me);
            s3 += exp_d(2.0 * lw);
        }
    }
    if (smoothed)
        for (int j = c; j < M; j += 16) {
            const double lw = tail_x[j] - lse;
            s2 += exp_d((lw + tail_ll[j]) - me);
            s3 += exp_d(2.0 * lw);
        }
    o.elpd = me + log(row16_sum(s2));
    o.wess = 1.0 / row16_sum(s3);
    return o;
}

}  // namespace epx
