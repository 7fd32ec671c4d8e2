// Private to libepx.so: the context behind the opaque epx_ctx of include/epx.h, shared by
// epx_api.hip (entry points), epx_draws.h (where an entry that post-processes draws finds them, and how it names
// parameters), epx_update.h (what the update stage decides on the host) and epx_comm.hip (the in-library RCCL binding).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <vector>

#include "../../include/epx.h"
#include "nuts_geometry.h"

// error message kept per thread, returned by epx_last_error(); always returns -1
int epx_fail(const char *fmt, ...);
#define fail epx_fail

#define HIPCHK(x)                                                                         \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define CTX(c)                                      \
    if (!(c)) return fail("null context");          \
    HIPCHK(hipSetDevice((c)->device));

// A device array of n elements of T that frees itself: every device allocation of the library is one.  It converts to
// T * where the array is used.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;

    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    operator T *() const { return p; }

    void release() {
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
    }
    // exactly `want` elements (room for one at least); the old array is freed first
    hipError_t alloc(size_t want) {
        release();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), (want ? want : 1) * sizeof(T));
        if (e == hipSuccess) n = want;
        else p = nullptr;
        return e;
    }
    // at least `want` elements: free, then allocate (peak memory: the new array alone)
    hipError_t grow(size_t want) { return want <= n ? hipSuccess : alloc(want); }
    // at least `want` elements: allocate first and keep the old array if that fails (the sticky error is cleared)
    bool try_grow(size_t want) {
        if (want <= n) return true;
        T *q = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(&q), want * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        release();
        p = q; n = want;
        return true;
    }
};

// Declared in front of the first queued copy that reads or writes caller or stack memory, behind the host buffers of such
// copies: whichever way the entry is left, the stream has been synchronised.  The good path ends with sync.finish().
struct StreamSync {
    hipStream_t stream;
    bool pending = true;
    ~StreamSync() { if (pending) (void)hipStreamSynchronize(stream); }
    int finish() {
        pending = false;
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
};

static const size_t LDS_CAP = epx::lds_capacity();

// A kernel that asks for more dynamic LDS than the default 64 KiB has to be told so before its launch
template <typename K>
int set_lds(K kern, size_t bytes) {
    if (bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return fail("hipFuncSetAttribute(%zu): %s", bytes, hipGetErrorString(e));
    }
    return 0;
}

// Queues a kernel that takes its argument struct by value, with `lds` bytes of dynamic LDS, and checks the launch
template <typename Args>
int launch(void (*kern)(Args), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args &a) {
    if (set_lds(kern, lds)) return -1;
    hipLaunchKernelGGL(kern, grid, block, lds, stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

struct epx_ctx {
    int device = 0, model = 0, K = 0, D = 0, d = 0, P = 0;
    int64_t N = 0;
    hipStream_t stream = nullptr;
    std::vector<int64_t> k_lim;
    // multi-group sites (K < J): groups per site, device copies of the prefix sums / row limits
    std::vector<int> g_cnt;
    std::vector<int> site_g0;       // K + 1: the first group of every site among all groups (one each without g_cnt)
    DevBuf<int> site_g0_d;
    DevBuf<int64_t> g_lim_d;
    std::vector<int64_t> g_lim;     // host copy of the groups' row limits (epx_draws.h: cut_ctx_rows cuts work items along them)
    int multi = 0, ng_max = 0, nt_max = 0, pg = 0;
    int n_max = 0;
    // device buffers
    DevBuf<int64_t> k_lim_d;
    DevBuf<double> X;
    DevBuf<uint8_t> y;
    DevBuf<int> y32;
    DevBuf<double> yd;              // real responses (Gaussian-likelihood family), else NULL
    int gauss = 0;
    DevBuf<double> Q0, r0, Q, r, S, m;
    DevBuf<double> Qi, ri, Qi2, ri2, dQi, dri;
    DevBuf<double> cav_Om, cav_mu;
    DevBuf<double> tilt_mean, tilt_scatter;
    // epx_set_draw_reuse: the cavities the sites of the last sampling call were sampled against (K x d x d, K x d, no
    // padding), the sites they cover, and the buffers of epx_reweight_batch: the caller's old cavities, the records
    int reuse_on = 0, snap_k0 = 0, snap_count = 0;
    DevBuf<double> drawn_Om, drawn_mu, rw_old, rw_out;
    DevBuf<uint8_t> flags;
    DevBuf<int> iflags;             // [4]
    DevBuf<double> packed, partial; // sums
    int nslice = 0;
    DevBuf<double> dense_ws;        // global workspace for dense kernels (lazily sized)
    // sampler buffers (lazily sized)
    int s_chains = 0, s_nkeep = 0;
    int drawn_k0 = 0, drawn_count = 0;   // sites the last sampling call covered: whose block of `draws` is current
    DevBuf<double> draws, last, chain_stats, site_stats, stack;
    DevBuf<double> team_passes;     // K: row-team passes of the last sampling call per site (layout 7; 0 elsewhere)
    DevBuf<int64_t> seeds_d;
    DevBuf<double> dbg;             // [1+P] lp, grad ; [P] theta (test hook)
    DevBuf<int64_t> dbg_seed;
    DevBuf<double> inj;             // draws the caller passed in place of the sampler's (epx_draws.h: upload_draws; epx_moments_batch)
    DevBuf<double> named_out;       // epx_named_moments: [mean | M2] records of the call
    DevBuf<double> pooled_ws;       // epx_pooled_moments: [partial tiles | partial sums | scatter | sum | centre]
    DevBuf<double> pred_ws;         // epx_predict: [new rows (n x D) | responses (n) | results (n x EPX_PR_COUNT)]
    DevBuf<int> pred_iws;           // ... [workgroup records (4 ints each) | sorted position -> row (n)]
                                    // (epx_predict_order_stats: [new rows | order statistics (n x n_ranks)] and [work items |
                                    // sorted position -> row | the rows' stream indices (n)] in the same two)
    DevBuf<double> loo_ws;          // epx_loo: [results (rows x EPX_LO_COUNT) | log-likelihood slabs, one per workgroup, when LDS is too small]
    DevBuf<double> ppc_ws;          // epx_ppc: [per-draw sums (groups x 3 x S) | group records | site records (x EPX_PC_COUNT)]
    DevBuf<double> ev_ws;           // epx_site_evidence: [proposal fits | terms l1, l2 | records (x EPX_EV_COUNT) | proposal draws, when asked for]
    DevBuf<double> diag_out;        // epx_draw_diagnostics: the call's records (count x P x EPX_DG_COUNT)
    DevBuf<double> rank_out;        // epx_draw_rank_diagnostics: the call's records (count x P x EPX_RD_COUNT)
    DevBuf<double> order_out;       // epx_named_order_stats: the call's order statistics (count x L x n_ranks)
    DevBuf<unsigned long long> count_ws;   // epx_pooled_count_pass: [histograms (L x n_targets x 256) | NaN counts (L) | prefixes (L x n_targets)]
    int has_last = 0;
    int nsamp = 0;                 // draws per site of the last tilted/moments call
    double last_df = 0.0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t stream2 = nullptr;  // second queue of a split sampling launch (epx_set_site_split)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int split_n = 0, last_split = 0, n_cu = 0;
    DevBuf<unsigned long long> stamps;  // diagnostic build: records of 8 cycle sums ...
    size_t stamps_last = 0;             // ... and how many the last sampling call wrote
    int last_layout = 0;
    DevBuf<int> order_d;
    int order_n = 0;
    int last_segments = 0;
    DevBuf<double> ckpt;
    // piece queue (epx_set_piece_queue): transitions per claim (0: off), predicted work per transition of the sites
    int dyn_len = 0, dyn_has_rate = 0;
    DevBuf<double> dyn_rate;
    DevBuf<int> dyn_words;          // [progress (K) | busy (K)]
    DevBuf<double> sweep_buf;       // damping sweep: target block + ndf x 5 criteria
    DevBuf<double> carry_eps, carry_metric;   // adapt = carry: K x chains step sizes, K x P diagonal metrics (lazily sized)
    int carry_chains = 0;                     // chains the history was recorded with (0: none)
    DevBuf<double> min_eig;         // force-pd fallback: smallest eigenvalue per site (K)
    // in-library RCCL binding (epx_comm.hip); comm == nullptr: single rank
    void *comm = nullptr;           // ncclComm_t
    int comm_rank = 0, comm_size = 0;
    int (*comm_ext)(double *, long long, int, void *) = nullptr;   // host transport given by the caller (epx_comm_init_host) ...
    void *comm_ext_user = nullptr;                                 // ... used instead of RCCL when set
    DevBuf<double> comm_stage;      // device staging of the small host-side collectives
    DevBuf<int> err_flag;           // device word the sampler kernels set when a hand-off spin gives up
    // epx_sample_piece (test hook): one piece of ONE transition from injected checkpoint records
    int hook_t0 = 0;                    // > 0 while such a call runs
    const double *hook_in = nullptr;    // host: K x chains records (csrc/epx_pieces.h layout)
    double *hook_out = nullptr;         // host: the records the piece leaves at boundary hook_t0 + 1
    // per-transition trace of the sampler (epx_set_trace, test hook): the first trace_sites sites of a sampling call
    int trace_sites = 0, trace_chains = 0, trace_iter = 0, trace_last_sites = 0;     // (trace_last_sites: what the last sampling call recorded)
    DevBuf<double> trace;

    epx_ctx() = default;
    epx_ctx(const epx_ctx &) = delete;
    epx_ctx &operator=(const epx_ctx &) = delete;
    // (the device arrays free themselves behind this, as members; the caller has made the context's device current)
    ~epx_ctx() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (stream2) (void)hipStreamDestroy(stream2);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

