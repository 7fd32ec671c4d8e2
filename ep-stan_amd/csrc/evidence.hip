// The site normaliser of EP by bridge sampling, from the draws the sampler left in device memory (include/epx.h,
// epx_site_evidence, states the definition; evidence.site_evidence_host restates it in NumPy).  Three kernels, one
// workgroup of four waves per site in each, stream-ordered; nothing is merged across workgroups and there are no
// floating-point atomics, so a site's record has the same bits on every call, whichever other sites are in the call.
//
// k_ev_fit.    The Gaussian proposal of a site from the fit set F (the first half of every chain): the mean, one thread
//              per coordinate adding the draws in order; the centred scatter in a second pass on v_mfma_f64_16x16x4_f64
//              tiles (operand layout: k_pooled_partial, pooled_moments.hip) -- a wave owns a pair of 16-column tiles for
//              all draws, so no tile is merged across waves; the packed Cholesky factor in LDS, column by column.  m, L
//              and sum log L_ii go to the context's workspace with a flag: 0 where a pivot was numerically <= 0 or
//              not finite.
// k_ev_terms   (evidence_terms.inc, compiled with predict.hip because it walks predict_tile.h's row tile).  l1 of the N1
//              estimation draws and l2 of N2 = N1 proposal draws, in slabs of 16 columns: a column's record theta is
//              built in LDS (a copy of the draw, or m + L z with z from the samplers' Philox stream at kind K_BRIDGE)
//              with the quadratic forms of the proposal density and of the cavity and the latents' prior, then the
//              site's rows go through the row-tile walk and are added per column as k_ppc adds them.
// k_ev_bridge. l1 and l2 in LDS; the iteration in log space, every sum a thread's own terms in increasing index, then
//              row16_sum and the 16 rows in order (wg_reduce); the error estimate; the k-hat of the proposal's
//              importance ratios by psis_smooth (psis.h) on 16 lanes.
#include "evidence.h"
#include "psis.h"

namespace epx {

typedef double v4d __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256)
k_ev_fit(EvidenceArgs a) {
    extern __shared__ __attribute__((aligned(16))) double ev_lds[];
    const int P = a.m.P, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double *Lp = ev_lds, *mv = Lp + evidence_packed(P);
    double *diag = mv + P;                               // the diagonal of C, against which a pivot is judged
    int &bad = *reinterpret_cast<int *>(diag + P);       // (in the dynamic region: a static would shift its base)
    const int j0 = blockIdx.x, k = a.k0 + j0, Pk = ev_coords(a, k), nF = a.nh * a.chains;
    const double *TH = a.draws + (size_t)j0 * a.S * P;
    double *fit = a.fit + (size_t)j0 * evidence_fit_doubles(P);

    if (tid == 0) bad = 0;
    for (int i = tid; i < Pk; i += 256) {
        double s = 0.0;
        for (int f = 0; f < nF; ++f) s += TH[(size_t)ev_fit_draw(a, f) * P + i];
        mv[i] = s / (double)nF;
    }
    __syncthreads();
    // the centred scatter: pair (ti >= tj) of 16-column tiles, a wave takes pairs wave, wave + 4, ...
    const int nt = (Pk + 15) / 16, npair = nt * (nt + 1) / 2, kq = lane >> 4;
    for (int pr = wave; pr < npair; pr += 4) {
        int ti = 0, rem = pr;
        while (rem > ti) { rem -= ti + 1; ++ti; }
        const int tj = rem, ia = ti * 16 + (lane & 15), ib = tj * 16 + (lane & 15);
        const bool ha = ia < Pk, hb = ib < Pk;
        const double ca = ha ? mv[ia] : 0.0, cb = hb ? mv[ib] : 0.0;
        v4d acc = {0.0, 0.0, 0.0, 0.0};
        for (int f0 = 0; f0 < nF; f0 += 4) {
            const int f = f0 + kq;
            double av = 0.0, bv = 0.0;
            if (f < nF) {
                const double *th = TH + (size_t)ev_fit_draw(a, f) * P;
                if (ha) av = th[ia] - ca;
                if (hb) bv = th[ib] - cb;
            }
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {                   // element (row kq + 4 r of tile ti, column lane & 15 of tile tj)
            const int i = ti * 16 + kq + 4 * r, j = tj * 16 + (lane & 15);
            if (i < Pk && j <= i) Lp[ev_tri(i, j)] = acc[r] / (double)(nF - 1);
        }
    }
    __syncthreads();
    for (int i = tid; i < Pk; i += 256) diag[i] = Lp[ev_tri(i, i)];
    __syncthreads();
    // packed Cholesky, right-looking: the pivot, the column, the trailing update by (row tid >> 4, column tid & 15) + 16 ...
    double sumlog = 0.0;
    const double tiny = (double)Pk * 0x1p-50;            // a pivot that rounding alone leaves of an exact zero
    for (int j = 0; j < Pk; ++j) {
        const double piv = Lp[ev_tri(j, j)];
        if (!(piv > tiny * diag[j]) || !isfinite(piv)) { // (the same value in every thread: a uniform exit)
            if (tid == 0) bad = 1;
            break;
        }
        const double ljj = sqrt(piv);
        sumlog += log(ljj);
        __syncthreads();                                 // every thread has read the pivot
        if (tid == 0) Lp[ev_tri(j, j)] = ljj;
        for (int i = j + 1 + tid; i < Pk; i += 256) Lp[ev_tri(i, j)] /= ljj;
        __syncthreads();
        for (int i = j + 1 + (tid >> 4); i < Pk; i += 16) {
            const double lij = Lp[ev_tri(i, j)];
            for (int c = j + 1 + (tid & 15); c <= i; c += 16) Lp[ev_tri(i, c)] -= lij * Lp[ev_tri(c, j)];
        }
        __syncthreads();
    }
    __syncthreads();
    for (int i = tid; i < P; i += 256) fit[i] = i < Pk ? mv[i] : 0.0;
    const int nl = (int)evidence_packed(P), nlk = (int)evidence_packed(Pk);
    for (int i = tid; i < nl; i += 256) fit[P + i] = i < nlk ? Lp[i] : 0.0;
    if (tid == 0) {
        fit[P + nl] = sumlog;
        fit[P + nl + 1] = bad ? 0.0 : 1.0;
    }
}

// op over the workgroup of a value per thread that the 16 lanes of a row have reduced already: the 16 rows through LDS, in
// a fixed order (predict_tile.h's wg_reduce, restated here: this file does not walk the row tile)
template <class Op>
__device__ __forceinline__ double wg_reduce(double v, double *scr, Op op) {
    __syncthreads();
    if ((threadIdx.x & 15) == 0) scr[threadIdx.x >> 4] = v;
    __syncthreads();
    double o = scr[0];
    for (int i = 1; i < 16; ++i) o = op(o, scr[i]);
    return o;
}

// log sum exp over i < N of term(i), about its largest term: all 256 threads; tmp: N doubles of LDS
template <class F>
__device__ inline double ev_lse(int N, F term, double *tmp, double *scr) {
    const int tid = threadIdx.x;
    double mx = -INFINITY;
    for (int i = tid; i < N; i += 256) {
        const double v = term(i);
        tmp[i] = v;
        mx = fmax(mx, v);
    }
    mx = wg_reduce(row16_max(mx), scr, [](double x, double y) { return fmax(x, y); });
    double s = 0.0;
    for (int i = tid; i < N; i += 256) s += exp(tmp[i] - mx);
    s = wg_reduce(row16_sum(s), scr, [](double x, double y) { return x + y; });
    return mx + log(s);
}
__device__ inline double ev_lse2(double x, double y) {
    const double t = fmax(x, y);
    return t + log(exp(x - t) + exp(y - t));
}
// mean and variance (divisor N - 1, centred in a second pass) of term(i), i < N: all 256 threads
template <class F>
__device__ inline void ev_mean_var(int N, F term, double *tmp, double *scr, double &mean, double &var) {
    const int tid = threadIdx.x;
    const auto add = [](double x, double y) { return x + y; };
    double s = 0.0;
    for (int i = tid; i < N; i += 256) {
        const double v = term(i);
        tmp[i] = v;
        s += v;
    }
    mean = wg_reduce(row16_sum(s), scr, add) / (double)N;
    double q = 0.0;
    for (int i = tid; i < N; i += 256) {
        const double dv = tmp[i] - mean;
        q += dv * dv;
    }
    var = wg_reduce(row16_sum(q), scr, add) / (double)(N - 1);
}

__global__ void __launch_bounds__(256)
k_ev_bridge(EvidenceArgs a) {
    extern __shared__ __attribute__((aligned(16))) double ev_lds[];
    const int N1 = a.N1, tid = threadIdx.x, j0 = blockIdx.x, P = a.m.P;
    double *l1 = ev_lds, *l2 = l1 + N1, *nl2 = l2 + N1, *tmp1 = nl2 + N1, *tmp2 = tmp1 + N1;
    double *pscr = tmp2 + N1, *scr = pscr + psis_scratch_doubles(a.M);
    const double *terms = a.terms + (size_t)j0 * 2 * N1;
    double *o = a.out + (size_t)j0 * EPX_EV_COUNT;
    const double ok = a.fit[(size_t)j0 * evidence_fit_doubles(P) + P + evidence_packed(P) + 1];
    const auto add = [](double x, double y) { return x + y; };

    double nbad = 0.0;
    for (int i = tid; i < N1; i += 256) {
        const double x = terms[i], y = terms[N1 + i];
        l1[i] = x; l2[i] = y; nl2[i] = -y;
        nbad += (isfinite(x) && isfinite(y)) ? 0.0 : 1.0;
    }
    nbad = wg_reduce(row16_sum(nbad), scr, add);
    if (ok == 0.0 || nbad != 0.0) {                       // (uniform)
        if (tid == 0) {
            o[EPX_EV_LOGZ] = o[EPX_EV_LOGZ_IS] = o[EPX_EV_RE2] = o[EPX_EV_KHAT] = NAN;
            o[EPX_EV_ITERS] = 0.0;
            o[EPX_EV_N1] = (double)N1;
        }
        return;
    }
    const double n1 = (double)N1, n2 = (double)N1, ls1 = log(n1 / (n1 + n2)), ls2 = log(n2 / (n1 + n2));
    const double s1 = n1 / (n1 + n2), s2 = n2 / (n1 + n2);
    const double rho0 = ev_lse(N1, [&](int i) { return l2[i]; }, tmp1, scr) - log(n2);
    double rho = rho0;
    int iters = 1001;
    for (int t = 1; t <= 1000; ++t) {
        const double b = ls2 + rho;
        const double num = ev_lse(N1, [&](int i) { return l2[i] - ev_lse2(ls1 + l2[i], b); }, tmp1, scr) - log(n2);
        const double den = ev_lse(N1, [&](int i) { return -ev_lse2(ls1 + l1[i], b); }, tmp2, scr) - log(n1);
        const double next = num - den;
        const bool done = fabs(next - rho) <= 1e-10;      // (the same bits in every thread)
        rho = next;
        if (done) { iters = t; break; }
    }
    double m1, v1, m2, v2;
    ev_mean_var(N1, [&](int i) { return 1.0 / (s1 * exp(l1[i] - rho) + s2); }, tmp1, scr, m1, v1);
    ev_mean_var(N1, [&](int i) { const double ex = exp(l2[i] - rho); return ex / (s1 * ex + s2); }, tmp2, scr, m2, v2);
    double khat = INFINITY;
    if (tid < 16) khat = psis_smooth(nl2, N1, a.M, a.mfit, pscr, tid, nullptr).khat;
    if (tid == 0) {
        o[EPX_EV_LOGZ] = rho;
        o[EPX_EV_LOGZ_IS] = rho0;
        o[EPX_EV_ITERS] = (double)iters;
        o[EPX_EV_RE2] = v2 / (n2 * (m2 * m2)) + v1 / (n1 * (m1 * m1));
        o[EPX_EV_KHAT] = khat;
        o[EPX_EV_N1] = n1;
    }
}

}  // namespace epx
