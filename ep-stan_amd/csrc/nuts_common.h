// Pieces shared by the sampler kernels (nuts.hip, nuts_duo.hip, nuts_stream.hip): the register layout
// of a length-P vector (element e in lane e % 64, register e / 64), its global-memory twin, the transposing
// butterfly, and the chain's scaffolding around nuts_state_machine.inc -- how a run starts (initial position,
// teacher-forced or carried step size and metric), the reduction of the leaf energy errors, the checkpoint
// record of a pieced launch and the chain's final record.  The scalars of the chain themselves, with the warm-up
// windows, are declarations in the kernel's scope: nuts_chain_state.inc.
#pragma once
#include "epx_device.h"
#include "epx_kernels.h"

// In-kernel cycle stamps exist only in the diagnostic build (-DEPX_STAMPS); its run time is never
// quoted, only the shares of the segments (scripts/stamps.py, scripts/stamps_stream.py).  What the slots mean
// is the kernel's business; TSTAMP is a second set of slots for a finer split.
#ifdef EPX_STAMPS
#define STAMP(i)                                                                   \
    do {                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                         \
        unsigned long long t_ = __builtin_amdgcn_s_memtime();                      \
        __builtin_amdgcn_s_waitcnt(0xC07F);                                        \
        tacc[i] += t_ - tprev; tprev = t_;                                         \
        __builtin_amdgcn_sched_barrier(0);                                         \
    } while (0)
#define STAMP_INIT unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long tprev = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xC07F)
#define TSTAMP(i)                                                                  \
    do {                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                         \
        unsigned long long t_ = __builtin_amdgcn_s_memtime();                      \
        __builtin_amdgcn_s_waitcnt(0xC07F);                                        \
        tdet[i] += t_ - tprev2; tprev2 = t_;                                       \
        __builtin_amdgcn_sched_barrier(0);                                         \
    } while (0)
#define TSTAMP_INIT unsigned long long tdet[8] = {0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long tprev2 = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xC07F)
#else
#define STAMP(i) do { } while (0)
#define STAMP_INIT do { } while (0)
#define TSTAMP(i) do { } while (0)
#define TSTAMP_INIT do { } while (0)
#endif

namespace epx {

template <int NV> struct Vec { double v[NV]; };

#define FORV _Pragma("unroll") for (int i = 0; i < NV; ++i)

template <int NV>
__device__ inline double gatherV(const Vec<NV> &x, int e) {
    double r = 0.0;
    FORV {
        const double t = __shfl(x.v[i], e & 63, 64);
        if ((e >> 6) == i) r = t;
    }
    return r;
}
// element e (wave-uniform index) as a scalar
template <int NV>
__device__ inline double elemU(const Vec<NV> &x, int e) {
    double r = 0.0;
    FORV { if ((e >> 6) == i) r = readlane_d(x.v[i], e & 63); }
    return r;
}

// A length-P vector kept in global memory behind the same `.v[i]` syntax (element e of lane e % 64 at
// b[e]): for the vectors of the tree bookkeeping that change once per subtree or per transition.  `b`
// is wave-uniform, so every access is `saddr + lane * 8 + immediate`.
// GVec<true> (nuts_duo.hip): elements beyond the vector's length `len` are 0 and not stored (fewer cache lines per
// vector).  GVec<false> (nuts_stream.hip) stores whole 64-lane rows; its specialisations carry neither the length nor
// the per-element flag -- as dead members of the one struct they cost the streaming kernels their schedule
// (profiles/chain_scaffolding_identity.txt).
template <bool MASKED> struct GRef {
    gdouble *p; bool ok;
    __device__ operator double() const { return ok ? *p : 0.0; }
    __device__ const GRef &operator=(double x) const { if (ok) *p = x; return *this; }
    __device__ const GRef &operator=(const GRef &o) const { const double x = o; if (ok) *p = x; return *this; }
    __device__ const GRef &operator+=(double x) const { if (ok) *p = *p + x; return *this; }
};
template <> struct GRef<false> {
    gdouble *p;
    __device__ operator double() const { return *p; }
    __device__ const GRef &operator=(double x) const { *p = x; return *this; }
    __device__ const GRef &operator=(const GRef &o) const { const double x = *o.p; *p = x; return *this; }
    __device__ const GRef &operator+=(double x) const { *p = *p + x; return *this; }
};
template <bool MASKED> struct GIdx {
    gdouble *b; int lane, len;
    __device__ GRef<MASKED> operator[](int i) const { return GRef<MASKED>{b + (lane + 64 * i), lane + 64 * i < len}; }
};
template <> struct GIdx<false> { gdouble *b; int lane; __device__ GRef<false> operator[](int i) const { return GRef<false>{b + (lane + 64 * i)}; } };
template <bool MASKED> struct GVec { GIdx<MASKED> v; };
// A wave-uniform scalar of the bookkeeping kept in the chain's global store: the adaptation state and the run's
// statistics are touched once per transition -- as registers they would be live through every leapfrog
struct GScal {
    gdouble *p;
    __device__ operator double() const { return *p; }
    __device__ const GScal &operator=(double x) const { *p = x; return *this; }
    __device__ const GScal &operator=(const GScal &o) const { const double x = *o.p; *p = x; return *this; }
    __device__ const GScal &operator+=(double x) const { *p = *p + x; return *this; }
};
struct RScal {            // the same interface on a register
    double x;
    __device__ operator double() const { return x; }
    __device__ RScal &operator=(double v) { x = v; return *this; }
    __device__ RScal &operator+=(double v) { x += v; return *this; }
};
__device__ inline void ck_assign(GScal &x, double v) { x = v; }
__device__ inline void ck_assign(RScal &x, double v) { x = v; }
enum { GV_QS, GV_GS, GV_PQ, GV_PP, GV_PG, GV_MQ, GV_MP, GV_MG, GV_RHO, GV_PSP, GV_PSM, GV_WMEAN, GV_WM2, GV_BQ, GV_BG,
       GV_SCAL,                 // one vector's worth of scalars (GScal; nuts_duo.hip only: the streaming kernel's store ends here)
       GV_COUNT };
// the fifteen cold vectors of a chain handed to the kernel's `bind(vector, its place in the store, lane)`
#define EPX_BIND_COLD(ln)                                                                              \
    bind(qs, GV_QS, ln); bind(gs, GV_GS, ln); bind(pq, GV_PQ, ln); bind(pp, GV_PP, ln); bind(pg, GV_PG, ln); \
    bind(mq, GV_MQ, ln); bind(mp, GV_MP, ln); bind(mg, GV_MG, ln); bind(rho, GV_RHO, ln);                 \
    bind(psp, GV_PSP, ln); bind(psm, GV_PSM, ln); bind(wmean, GV_WMEAN, ln); bind(wm2, GV_WM2, ln); \
    bind(bq, GV_BQ, ln); bind(bg, GV_BG, ln)

__device__ inline gdouble *uniform_ptr(double *p) {
    const unsigned long long u = (unsigned long long)p;
    const unsigned lo32 = __builtin_amdgcn_readfirstlane((unsigned)u);
    const unsigned hi32 = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return reinterpret_cast<gdouble *>((uintptr_t)(((unsigned long long)hi32 << 32) | lo32));
}

template <int DP> struct Log2 { static constexpr int v = 1 + Log2<DP / 2>::v; };
template <> struct Log2<1> { static constexpr int v = 0; };

enum { MODE_INIT = 0, MODE_SS = 1, MODE_TREE = 2 };

// Transposing reduction of CNT per-lane partial sums over the 64 lanes of a wave:
// each stage halves the values a lane carries and doubles the lanes summed, so
// CNT values cost CNT-1 exchanges (not 6*CNT).  Stage with selector bit B keeps
// the half of the values chosen by the lane's own bit B and receives the same
// half from a partner lane whose bit B differs.  Fully static indexing.
template <int CNT, int B>
__device__ inline void butterfly(double *acc, int lane) {
    if constexpr (CNT > 1) {
        if constexpr (B >= 4) {
#pragma unroll
            for (int j = 0; j < CNT / 2; ++j) acc[j] = swap_add_d<B>(acc[j], acc[j + CNT / 2]);
        } else {
            const bool upper = (lane >> B) & 1;
#pragma unroll
            for (int j = 0; j < CNT / 2; ++j) {
                const double send = upper ? acc[j] : acc[j + CNT / 2];
                const double keep = upper ? acc[j + CNT / 2] : acc[j];
                acc[j] = keep + partner_d<B>(send, lane);
            }
        }
        butterfly<CNT / 2, B - 1>(acc, lane);
    } else if constexpr (B >= 0) {
        acc[0] += partner_d<B>(acc[0], lane);
        butterfly<1, B - 1>(acc, lane);
    }
}

// ---------------------------------------------------------------------------
// The chain's scaffolding around nuts_state_machine.inc, one definition each for k_nuts, k_nuts_spec's bookkeeping
// wave (nuts.hip), duo_piece (nuts_duo.hip) and stream_piece (nuts_stream.hip).
//
// All but the first are MACROS over the bare names of the chain's scope (nuts_chain_state.inc, and the kernel's `a`, k,
// sb, chain, P, key, NV and vectors), like the state machine itself: the same text in the same place compiles to the
// same instructions.  As force-inlined functions each of them -- even the six lines of the warm-up windows, even the
// uniform(-2, 2) draw inside the state machine -- came out of the inliner with its instructions in another order, and
// from there every sampler kernel got another schedule and another register allocation
// (profiles/chain_scaffolding_identity.txt).  Parameters are only what differs between the kernels.
// They are STATEMENT SEQUENCES, not expressions: several of them are not wrapped in braces because they declare names
// for the code behind them (teacher, carry, ckv), so each stands as a statement of its own in a block -- never as the
// unbraced body of an if / for -- once per scope.  That is how the four kernels use them, and the only safe way.
// The checkpoint blocks need epx_pieces.h (ck_load, ck_store, EPX_CK_LIST): the kernels that use them include it.

// Reduce the buffered leaf energy errors (lanes 0..cnt-1 of dhb) into the running log-sum-weight (lw_m + log lw_s) and
// the accept statistic.  LEAN: the lean exp of epx_device.h (row team: a wave that completes a subtree keeps the three
// other chains and the row team waiting at the pass's barrier, and libm's exp is ~10 x the instructions)
template <bool LEAN>
__device__ __forceinline__ void flush_leaf_dh(int lane, int cnt, double dhb, double &lw_m, double &lw_s, double &sum_metro) {
    auto ex = [](double x) -> double { if constexpr (LEAN) return exp_d(x); else return exp(x); };
    const bool ok = lane < cnt;
    const double dh = ok ? dhb : -INFINITY;
    const double mb = wave_max(dh);
    const double m_new = fmax(lw_m, mb);
    double w = 0.0, me = 0.0;
    if (ok) {
        w = (m_new == -INFINITY) ? 0.0 : ex(dh - m_new);
        me = dh > 0 ? 1.0 : ex(dh);
    }
    wave_sum2(w, me);
    const double scale = (lw_m == -INFINITY) ? 0.0 : ex(lw_m - m_new);
    lw_s = lw_s * scale + w;
    lw_m = m_new;
    sum_metro += me;
}

// Stan's uniform(-2, 2) start of element e_: draw try_ of the chain (Stan draws again, up to 100 times, until log
// density and gradient are finite: the retry of nuts_state_machine.inc).  Draw r of the chain is the Philox stream of
// the first one with r in its last counter word.
#define EPX_INIT_DRAW(q0_, e_, try_)                                                        \
    {                                                                                       \
        double u1, u2;                                                                      \
        rng_u2(key, 0, K_INIT, (uint32_t)((e_) >> 1), (uint32_t)(try_), u1, u2);            \
        q0_ = -2.0 + 4.0 * (((e_) & 1) ? u2 : u1);                                          \
    }
// Initial position of element e_ into q0_ (method.py:159 init / :404-406 init_prev): zeros (a.init_mode 1), the
// previous draws (2, lastp_), or the first uniform(-2, 2) draw (0); 0 beyond the vector's length P.
// (two statements, no braces: q0_ is the caller's variable; use as a statement in a braced block)
#define EPX_INIT_POSITION(q0_, e_, lastp_)                                                  \
    q0_ = 0.0;                                                                              \
    if ((e_) < P) {                                                                         \
        if (a.init_mode == 2) q0_ = (lastp_)[e_];                                           \
        else if (a.init_mode == 0) EPX_INIT_DRAW(q0_, e_, 0)                                \
    }

// Declares `teacher` and `carry` and loads what they stand for into eps, da_mu and inv_e.
// teacher: fixed step size / metric of the launch's chain (test hook: a.eps_in is set).
// carry: opt-in carried adaptation -- last call's step size of the chain, the site's pooled sample variances (the chain
// then keeps the metric it started with: only the step size is adapted).
// active_: the wave has a chain; ln_: its lane index; stride_: width of the records (a.P)
// (declares `teacher` and `carry` in the caller's scope, hence no braces: once per scope, as a statement of its own)
#define EPX_LOAD_TEACHER_CARRY(active_, ln_, stride_)                                                                   \
    const bool teacher = a.eps_in != nullptr;                                                                           \
    if (teacher && active_) {                                                                                           \
        eps = a.eps_in[(size_t)sb * a.chains + chain];                                                                  \
        if (a.inv_e_in) {                                                                                               \
            const double *ie = a.inv_e_in + ((size_t)sb * a.chains + chain) * stride_;                                  \
            FORV { const int e = ln_ + 64 * i; if (e < P) inv_e.v[i] = ie[e]; }                                         \
        }                                                                                                               \
    }                                                                                                                   \
    const bool carry = active_ && !teacher && a.carry_eps != nullptr && a.carry_eps[(size_t)k * a.chains + chain] > 0.0; \
    if (carry) {                                                                                                        \
        eps = a.carry_eps[(size_t)k * a.chains + chain];                                                                \
        da_mu = log(10.0 * eps);                                                                                        \
        const double *cm = a.carry_metric + (size_t)k * stride_;                                                        \
        FORV { const int e = ln_ + 64 * i; if (e < P) inv_e.v[i] = cm[e]; }                                             \
    }

// ---- checkpoint record of a pieced launch (epx_pieces.h): sample, Welford mean and sum of squares, metric (NV x 64
// each), then one line of scalars, EPX_CK_LIST's variable idx in lane idx.  The gradient at the sample is not kept: the
// piece that continues evaluates it again.
// element i (the FORV index) of the sample into q_i_, and of the Welford sums
#define EPX_CK_RESTORE_SAMPLE(ckp_, ln_, q_i_)                      \
    q_i_ = ck_load((ckp_) + (0 * NV + i) * 64 + ln_);               \
    wmean.v[i] = ck_load((ckp_) + (1 * NV + i) * 64 + ln_);         \
    wm2.v[i] = ck_load((ckp_) + (2 * NV + i) * 64 + ln_)
// the metric and the scalars; declares `ckv`, the line of scalars as it was read, in the caller's scope (no braces:
// once per scope, as a statement of its own in a braced block)
#define EPX_CK_GET(idx, x) ck_assign(x, readlane_d(ckv, idx));
#define EPX_CK_RESTORE_STATE(ckp_, ln_)                             \
    FORV inv_e.v[i] = ck_load((ckp_) + (3 * NV + i) * 64 + ln_);    \
    const double ckv = ck_load((ckp_) + 4 * NV * 64 + ln_);         \
    EPX_CK_LIST(EPX_CK_GET)
#define EPX_CK_PUT(idx, x) ck_line_ = ck_lane_ == (idx) ? (double)(x) : ck_line_;
#define EPX_CK_SAVE(ckp_, ln_)                                      \
    {                                                               \
        const int ck_lane_ = ln_;                                   \
        FORV {                                                      \
            ck_store((ckp_) + (0 * NV + i) * 64 + ck_lane_, qs.v[i]);      \
            ck_store((ckp_) + (1 * NV + i) * 64 + ck_lane_, wmean.v[i]);   \
            ck_store((ckp_) + (2 * NV + i) * 64 + ck_lane_, wm2.v[i]);     \
            ck_store((ckp_) + (3 * NV + i) * 64 + ck_lane_, inv_e.v[i]);   \
        }                                                           \
        double ck_line_ = 0.0;                                      \
        EPX_CK_LIST(EPX_CK_PUT)                                     \
        ck_store((ckp_) + 4 * NV * 64 + ck_lane_, ck_line_);        \
    }

// The chain's final record: its last sample (the next call's init_prev), for a failed chain its draws (all of them that
// sample), and the eight chain_stats.  len_: elements of the vectors that are written; stride_: width of the records (a.P)
#define EPX_WRITE_CHAIN_RECORD(ln_, len_, stride_)                                                                      \
    {                                                                                                                   \
        double *lastp = a.last + ((size_t)k * a.chains + chain) * stride_;                                              \
        FORV { const int e = ln_ + 64 * i; if (e < len_) lastp[e] = qs.v[i]; }                                          \
        if (failed) {                                                                                                   \
            for (int kk = 0; kk < a.nkeep; ++kk) {                                                                      \
                double *dst = a.draws + (((size_t)k * a.chains + chain) * a.nkeep + kk) * stride_;                      \
                FORV { const int e = ln_ + 64 * i; if (e < len_) dst[e] = qs.v[i]; }                                    \
            }                                                                                                           \
        }                                                                                                               \
        if (ln_ == 0) {                                                                                                 \
            double *st = a.chain_stats + ((size_t)k * a.chains + chain) * ST_COUNT;                                     \
            st[ST_STEPSIZE_MEAN] = a.iter > 0 && !failed ? eps_sum / a.iter : 0.0;                                      \
            st[ST_STEPSIZE_FINAL] = eps;                                                                                \
            st[ST_NLEAP] = nleap_tot;                                                                                   \
            st[ST_NGRAD] = ngrad;                                                                                       \
            st[ST_NDIV] = ndiv;                                                                                         \
            st[ST_ACCEPT_MEAN] = npost ? acc_sum / npost : 0.0;                                                         \
            st[ST_DEPTH_MEAN] = npost ? depth_sum / npost : 0.0;                                                        \
            st[ST_FAIL] = failed;                                                                                       \
        }                                                                                                               \
    }

// host side: how every sampler kernel is started -- the kernel is allowed `lds` bytes of dynamic LDS (beyond the 64 KB a
// kernel may have unasked), launched, and the launch's error returned (hipError_t as int)
template <class Kern>
static int launch_with_lds(Kern kern, int nblocks, int threads, size_t lds, hipStream_t stream, const NutsArgs &a) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(threads), lds, stream, a);
    return (int)hipGetLastError();
}

}  // namespace epx
