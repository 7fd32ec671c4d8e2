// C-ABI of libepx.so (include/epx.h): context management, host<->device
// copies and kernel launches.  No CPU fallback exists: without a HIP device
// every entry point fails with an error message.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <algorithm>
#include <vector>

#include "../../include/epx.h"
#include "epx_kernels.h"
#include "epx_pieces.h"
#include "psis.h"
#include "epx_ctx.h"
#include "epx_draws.h"
#include "epx_update.h"

using namespace epx;

static thread_local std::string g_err;

int epx_fail(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return -1;
}

const char *epx_last_error(void) { return g_err.c_str(); }

int epx_device_count(int *count) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; return fail("hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = c;
    return 0;
}

int epx_runtime_info(int device, int *hip_runtime_version, char *arch, int arch_len) {
    int v = 0;
    hipError_t e = hipRuntimeGetVersion(&v);
    if (e != hipSuccess) return fail("hipRuntimeGetVersion: %s", hipGetErrorString(e));
    if (hip_runtime_version) *hip_runtime_version = v;
    if (arch && arch_len > 0) {
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, device);
        if (e != hipSuccess) return fail("hipGetDeviceProperties(%d): %s", device, hipGetErrorString(e));
        snprintf(arch, (size_t)arch_len, "%s", prop.gcnArchName);
    }
    return 0;
}

int epx_device_synchronize(int device) {
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail("epx_device_synchronize(%d): %s", device, hipGetErrorString(e));
    return 0;
}

int epx_model_dims(int model, int D, int *dphi, int *npar) {
    int d, P;
    const int o = (model >= EPX_M1A_SG && model <= EPX_M5A_SG) ? 1 : 0;      // log sigma in front
    switch (model - (o ? EPX_M1A_SG : 0)) {
    case EPX_M1B_SG: d = D + 1; P = D + 2; break;
    case EPX_M2B_SG: d = 2; P = D + 3; break;
    case EPX_M3B_SG: d = D + 1; P = 2 * D + 2; break;
    case EPX_M4B_SG: case EPX_M5B_SG: d = 2 * D + 2; P = 3 * D + 3; break;
    default: return fail("unknown model id %d", model);
    }
    if (dphi) *dphi = d + o;
    if (npar) *npar = P + o;
    return 0;
}

int epx_comm_allreduce_dev(epx_ctx *c, double *buf, size_t n, int op);      // epx_comm.hip

// Queues one dense kernel (dense.hip) at dimension d: `grid` blocks of 256 threads, their work matrices in dynamic LDS or
// in `buf`, grown to `nblocks` slots (epx_update.h: DensePlan).  d, ld and ws of the argument struct are filled here.
template <typename Args>
static int launch_dense(void (*kern)(Args), int grid, hipStream_t stream, DevBuf<double> &buf, int d, int nblocks, Args &a) {
    const DensePlan p(d);
    HIPCHK(buf.grow(p.ws_doubles(nblocks)));            // (no doubles, no allocation, while the matrices are in LDS)
    a.d = d; a.ld = p.ld;
    a.ws.use_lds = p.in_lds; a.ws.global = p.in_lds ? nullptr : buf.p;
    return launch(kern, dim3(grid), dim3(256), p.lds_bytes, stream, a);
}

// A caller's array that may only be read goes up to the device; one that may be written is filled from it.
static hipError_t copy_host(double *dev, const double *host, size_t n) { return hipMemcpy(dev, host, n * 8, hipMemcpyHostToDevice); }
static hipError_t copy_host(double *dev, double *host, size_t n) { return hipMemcpy(host, dev, n * 8, hipMemcpyDeviceToHost); }

// The accessors' pair of synchronous copies between the caller's arrays Qh, rh (H: const double or double, as above) and records
// [k, k + count) of two device arrays (d x d and d doubles a record): each only if the caller gave its array.
template <typename H>
static int copy_pair(const epx_ctx *c, double *Qd, double *rd, size_t k, size_t count, H *Qh, H *rh) {
    const size_t d = c->d;
    if (Qh) HIPCHK(copy_host(Qd + k * d * d, Qh, count * d * d));
    if (rh) HIPCHK(copy_host(rd + k * d, rh, count * d));
    return 0;
}

// Queued: (Qo, ro) = (Qi, ri) + df (dQi, dri) over all sites -- the proposal of a trial, or in place the accepted update
static int queue_site_axpy(epx_ctx *c, double *Qo, double *ro, double df) {
    const size_t K = c->K, d = c->d;
    hipLaunchKernelGGL(k_axpy, dim3(1024), dim3(256), 0, c->stream, Qo, c->Qi, c->dQi, df, K * d * d);
    hipLaunchKernelGGL(k_axpy, dim3(64), dim3(256), 0, c->stream, ro, c->ri, c->dri, df, K * d);
    HIPCHK(hipGetLastError());
    return 0;
}

static int ctx_create(int device, int model, int K_local, int D, const int64_t *k_lim, const int32_t *g_cnt,
                      const int64_t *g_lim, const double *X, const int32_t *y, const double *yd, epx_ctx **out);

int epx_ctx_create(int device, int model, int K_local, int D, const int64_t *k_lim, const double *X,
                   const int32_t *y, epx_ctx **out) {
    return epx_ctx_create_groups(device, model, K_local, D, k_lim, nullptr, nullptr, X, y, out);
}

int epx_ctx_create_groups(int device, int model, int K_local, int D, const int64_t *k_lim, const int32_t *g_cnt,
                          const int64_t *g_lim, const double *X, const int32_t *y, epx_ctx **out) {
    if (out) *out = nullptr;
    if (model >= EPX_M1A_SG && model <= EPX_M5A_SG)
        return fail("model %d has real responses: use epx_ctx_create_real", model);
    return ctx_create(device, model, K_local, D, k_lim, g_cnt, g_lim, X, y, nullptr, out);
}

int epx_ctx_create_real(int device, int model, int K_local, int D, const int64_t *k_lim, const double *X,
                        const double *y, epx_ctx **out) {
    return epx_ctx_create_real_groups(device, model, K_local, D, k_lim, nullptr, nullptr, X, y, out);
}

int epx_ctx_create_real_groups(int device, int model, int K_local, int D, const int64_t *k_lim, const int32_t *g_cnt,
                               const int64_t *g_lim, const double *X, const double *y, epx_ctx **out) {
    if (out) *out = nullptr;
    if (model < EPX_M1A_SG || model > EPX_M5A_SG)
        return fail("model %d has 0/1 responses: use epx_ctx_create", model);
    return ctx_create(device, model, K_local, D, k_lim, g_cnt, g_lim, X, nullptr, y, out);
}

static int ctx_create(int device, int model, int K_local, int D, const int64_t *k_lim, const int32_t *g_cnt,
                      const int64_t *g_lim, const double *X, const int32_t *y, const double *yd, epx_ctx **out) {
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail("no HIP device available: libepx has no CPU fallback");
    if (device < 0 || device >= ndev) return fail("device %d out of range (%d devices)", device, ndev);
    int d, P;
    if (epx_model_dims(model, D, &d, &P)) return -1;
    if (K_local < 1) return fail("K_local must be >= 1");
    if (D < 1) return fail("D must be >= 1");
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<epx_ctx> c(new epx_ctx());          // (freed with all it holds on every early return)
    c->device = device; c->K = K_local; c->D = D; c->d = d; c->P = P;
    c->gauss = yd != nullptr;
    c->model = c->gauss ? model - EPX_M1A_SG : model;       // the kernels take the b-model id plus the family flag
    model = c->model;
    c->k_lim.assign(k_lim, k_lim + K_local + 1);
    c->N = k_lim[K_local] - k_lim[0];
    for (int k = 0; k < K_local; ++k) {
        const int64_t n = k_lim[k + 1] - k_lim[k];
        if (n < 1) return fail("site %d is empty", k);
        if (n > c->n_max) c->n_max = (int)n;
    }
    if (k_lim[0] != 0) return fail("k_lim[0] must be 0 (rows are rank-local)");
    // groups: tiles never straddle two groups, so the tile count of a site depends on them
    c->pg = model == EPX_M1B_SG ? 1 : 1 + D;
    c->multi = g_cnt != nullptr;
    c->ng_max = 1; c->nt_max = 1;
    std::vector<int> &g0 = c->site_g0;
    g0.assign((size_t)K_local + 1, 0);
    {
        int64_t gi = 0;
        for (int k = 0; k < K_local; ++k) {
            const int ng = g_cnt ? g_cnt[k] : 1;
            if (ng < 1) return fail("site %d has %d groups", k, ng);
            if (ng > c->ng_max) c->ng_max = ng;
            int nt = 0;
            for (int g = 0; g < ng; ++g) {
                const int64_t lo = g_cnt ? g_lim[gi + g] : k_lim[k], hi = g_cnt ? g_lim[gi + g + 1] : k_lim[k + 1];
                if (hi <= lo) return fail("group %d of site %d is empty", g, k);
                nt += (int)((hi - lo + 15) / 16);
            }
            if (g_cnt && (g_lim[gi] != k_lim[k] || g_lim[gi + ng] != k_lim[k + 1]))
                return fail("the groups of site %d do not cover its rows", k);
            if (nt > c->nt_max) c->nt_max = nt;
            gi += ng;
            g0[k + 1] = (int)gi;
        }
        if (g_cnt) {
            c->g_cnt.assign(g_cnt, g_cnt + K_local);
            c->g_lim.assign(g_lim, g_lim + gi + 1);
            c->P = d + c->ng_max * c->pg;           // record stride: the largest site
        }
    }
    HIPCHK(hipStreamCreate(&c->stream));
    HIPCHK(hipEventCreate(&c->ev0));
    HIPCHK(hipEventCreate(&c->ev1));
    {
        // own priority level = own hardware queue: normal-priority streams share 4 queues round-robin
        // by first use, and two streams on one queue run their kernels one after the other (measured:
        // scripts/probe/concurrent.hip)
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, hi));
    }
    HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    {
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, device));
        c->n_cu = prop.multiProcessorCount;
    }
    const size_t K = K_local, d2 = (size_t)d * d;
    HIPCHK(c->k_lim_d.alloc(K + 1));
    if (c->multi) {
        HIPCHK(c->site_g0_d.alloc(K + 1));
        HIPCHK(c->g_lim_d.alloc((size_t)g0[K] + 1));
        HIPCHK(hipMemcpy(c->site_g0_d, g0.data(), (K + 1) * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->g_lim_d, g_lim, ((size_t)g0[K] + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    // X carries a zeroed KiB behind the last row: the streaming sampler's row DMA reads full
    // 128-column images
    HIPCHK(c->X.alloc((size_t)c->N * D + 128));
    HIPCHK(hipMemset(c->X + (size_t)c->N * D, 0, 128 * sizeof(double)));
    HIPCHK(c->y.alloc((size_t)c->N));
    HIPCHK(c->y32.alloc((size_t)c->N));
    HIPCHK(c->Q0.alloc(d2)); HIPCHK(c->r0.alloc(d));
    HIPCHK(c->Q.alloc(d2)); HIPCHK(c->r.alloc(d));
    HIPCHK(c->S.alloc(d2)); HIPCHK(c->m.alloc(d));
    HIPCHK(c->Qi.alloc(K * d2)); HIPCHK(c->ri.alloc(K * d));
    HIPCHK(c->Qi2.alloc(K * d2)); HIPCHK(c->ri2.alloc(K * d));
    HIPCHK(c->dQi.alloc(K * d2)); HIPCHK(c->dri.alloc(K * d));
    // (64 columns of zeros behind the last site's cavity precision: the streaming sampler requests its columns a round
    // ahead, nuts_stream.hip)
    HIPCHK(c->cav_Om.alloc(K * d2 + (size_t)EPX_OM_PAD_COLS * d)); HIPCHK(c->cav_mu.alloc(K * d));
    HIPCHK(hipMemset(c->cav_Om + K * d2, 0, (size_t)EPX_OM_PAD_COLS * d * sizeof(double)));
    HIPCHK(c->tilt_mean.alloc(K * d)); HIPCHK(c->tilt_scatter.alloc(K * d2));
    HIPCHK(c->flags.alloc(K));
    HIPCHK(c->iflags.alloc(4));
    HIPCHK(c->min_eig.alloc(K));
    HIPCHK(c->err_flag.alloc(4));
    HIPCHK(hipMemset(c->err_flag, 0, 4 * sizeof(int)));
    HIPCHK(c->dbg.alloc(2 * (size_t)c->P + 1));
    HIPCHK(c->dbg_seed.alloc(1));
    const int len = 2 * (int)(d2 + d);
    c->nslice = K_local >= 64 ? 32 : 1;
    HIPCHK(c->packed.alloc((size_t)len + PACKED_EXTRA));
    HIPCHK(c->partial.alloc((size_t)len * c->nslice));
    HIPCHK(hipMemcpy(c->k_lim_d, k_lim, (K + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->X, X, (size_t)c->N * D * sizeof(double), hipMemcpyHostToDevice));
    if (c->gauss) {
        for (int64_t i = 0; i < c->N; ++i)
            if (!std::isfinite(yd[i])) return fail("y[%lld] is not finite", (long long)i);
        HIPCHK(c->yd.alloc((size_t)c->N));
        HIPCHK(hipMemcpy(c->yd, yd, (size_t)c->N * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemset(c->y, 0, (size_t)c->N));
        HIPCHK(hipMemset(c->y32, 0, (size_t)c->N * sizeof(int)));
    } else {
        std::vector<uint8_t> yb((size_t)c->N);
        for (int64_t i = 0; i < c->N; ++i) {
            if (y[i] != 0 && y[i] != 1) return fail("y[%lld] = %d is not 0/1", (long long)i, y[i]);
            yb[i] = (uint8_t)y[i];
        }
        HIPCHK(hipMemcpy(c->y, yb.data(), yb.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->y32, y, (size_t)c->N * sizeof(int), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemset(c->Qi, 0, K * d2 * 8)); HIPCHK(hipMemset(c->ri, 0, K * d * 8));
    HIPCHK(hipMemset(c->Qi2, 0, K * d2 * 8)); HIPCHK(hipMemset(c->ri2, 0, K * d * 8));
    HIPCHK(hipMemset(c->dQi, 0, K * d2 * 8)); HIPCHK(hipMemset(c->dri, 0, K * d * 8));
    HIPCHK(hipMemset(c->Q0, 0, d2 * 8)); HIPCHK(hipMemset(c->r0, 0, d * 8));
    HIPCHK(hipMemset(c->Q, 0, d2 * 8)); HIPCHK(hipMemset(c->r, 0, d * 8));
    HIPCHK(hipMemset(c->flags, 0, K));
    *out = c.release();
    return 0;
}

int epx_ctx_destroy(epx_ctx *c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    if (c->comm || c->comm_ext) (void)epx_comm_destroy(c);
    delete c;
    return 0;
}

int epx_set_prior(epx_ctx *c, const double *Q0, const double *r0) {
    CTX(c);
    return copy_pair(c, c->Q0, c->r0, 0, 1, Q0, r0);
}

static int check_range(epx_ctx *c, int k0, int count) {
    if (k0 < 0 || count < 1 || k0 + count > c->K) return fail("site range [%d,%d) outside [0,%d)", k0, k0 + count, c->K);
    return 0;
}

static int site_ptrs(epx_ctx *c, int which, double **Q, double **r) {
    switch (which) {
    case EPX_QI: *Q = c->Qi; *r = c->ri; return 0;
    case EPX_QI2: *Q = c->Qi2; *r = c->ri2; return 0;
    case EPX_DQI: *Q = c->dQi; *r = c->dri; return 0;
    }
    return fail("unknown site array %d", which);
}

// sites [k, k + count) of a site array to or from the caller's arrays (copy_pair)
template <typename H>
static int copy_sites(epx_ctx *c, int which, int k, int count, H *Qh, H *rh) {
    double *Q, *r;
    if (site_ptrs(c, which, &Q, &r)) return -1;
    return copy_pair(c, Q, r, k, count, Qh, rh);
}

int epx_set_sites(epx_ctx *c, int which, const double *QF, const double *rF) {
    CTX(c);
    return copy_sites(c, which, 0, c->K, QF, rF);
}

int epx_get_sites(epx_ctx *c, int which, double *QF, double *rF) {
    CTX(c);
    if (which == EPX_QI2) {
        // materialise the proposal Qi + df*dQi of the last trial (method.py:1071-1072)
        if (queue_site_axpy(c, c->Qi2, c->ri2, c->last_df)) return -1;
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return copy_sites(c, which, 0, c->K, QF, rF);
}

int epx_set_site(epx_ctx *c, int which, int k, const double *Qh, const double *rh) {
    CTX(c);
    if (check_range(c, k, 1)) return -1;
    return copy_sites(c, which, k, 1, Qh, rh);
}

int epx_get_site(epx_ctx *c, int which, int k, double *Qh, double *rh) {
    CTX(c);
    if (check_range(c, k, 1)) return -1;
    if (which == EPX_QI2) return fail("epx_get_site: use epx_get_sites for the proposal array");
    return copy_sites(c, which, k, 1, Qh, rh);
}

int epx_set_global(epx_ctx *c, const double *Q, const double *r) {
    CTX(c);
    return copy_pair(c, c->Q, c->r, 0, 1, Q, r);
}
int epx_get_global(epx_ctx *c, double *Q, double *r) {
    CTX(c);
    return copy_pair(c, c->Q, c->r, 0, 1, Q, r);
}

static int launch_cavity(epx_ctx *c, const double *Qs, const double *rs, const double *dQs,
                         const double *drs, double df, int k0, int count) {
    CavityArgs a;
    a.k0 = k0;
    a.Q = c->Q; a.r = c->r; a.Qsite = Qs; a.rsite = rs; a.dQsite = dQs; a.drsite = drs;
    a.site_stride = (size_t)c->d * c->d; a.rsite_stride = c->d; a.df = df;
    a.cav_Om = c->cav_Om; a.cav_mu = c->cav_mu; a.flags = c->flags;
    return launch_dense(k_cavity, count, c->stream, c->dense_ws, c->d, count, a);
}

// Queued: the cavities of the proposals Qi + df dQi, ri + df dri of sites [k0, k0 + count) against the global approximation
static int launch_proposal_cavities(epx_ctx *c, double df, int k0, int count) { return launch_cavity(c, c->Qi, c->ri, c->dQi, c->dri, df, k0, count); }

// The tail of the entries that leave per-site flags: the stream synchronised, then those of sites [k0, k0 + count) to the caller
static int fetch_flags(epx_ctx *c, int k0, int count, uint8_t *out) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (out) HIPCHK(hipMemcpy(out, c->flags + k0, count, hipMemcpyDeviceToHost));
    return 0;
}

int epx_cavity_batch(epx_ctx *c, int which, int k0, int count, uint8_t *posdef) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    if (which != EPX_QI && which != EPX_QI2) return fail("cavity needs EPX_QI or EPX_QI2");
    if (which == EPX_QI ? launch_cavity(c, c->Qi, c->ri, nullptr, nullptr, 0.0, k0, count)
                        : launch_proposal_cavities(c, c->last_df, k0, count)) return -1;
    return fetch_flags(c, k0, count, posdef);
}

int epx_cavity_site(epx_ctx *c, int k, const double *Q, const double *r, const double *Qi,
                    const double *ri, uint8_t *posdef) {
    CTX(c);
    if (check_range(c, k, 1)) return -1;
    // the caller's arrays become the context's state for this site (Worker.cavity
    // aliases Q, r: method.py:286-287)
    if (copy_pair(c, c->Q, c->r, 0, 1, Q, r)) return -1;
    if (copy_pair(c, c->Qi2, c->ri2, k, 1, Qi, ri)) return -1;
    if (launch_cavity(c, c->Qi2, c->ri2, nullptr, nullptr, 0.0, k, 1)) return -1;
    return fetch_flags(c, k, 1, posdef);
}

int epx_get_cavity(epx_ctx *c, int k, double *Mat, double *vec) {
    CTX(c);
    if (check_range(c, k, 1)) return -1;
    return copy_pair(c, c->cav_Om, c->cav_mu, k, 1, Mat, vec);
}

// ------------------------------------------------------------------ sampler
static int norm_opts(const epx_sampler_opts *o, epx_sampler_opts *n) {
    if (!o) return fail("null sampler options");
    *n = *o;
    if (n->chains < 1 || n->chains > 16) return fail("chains must be in 1..16 (got %d)", n->chains);
    if (n->iter < 1) return fail("iter must be >= 1");
    if (n->warmup < 0) n->warmup = n->iter / 2;                 // method.py:157,567-569
    if (n->warmup >= n->iter) return fail("warmup (%d) must be smaller than iter (%d)", n->warmup, n->iter);
    if (n->thin < 1) return fail("thin must be >= 1");
    if (n->max_depth <= 0) n->max_depth = 10;
    if (n->max_depth > MAX_DEPTH_CAP) return fail("max_depth > %d", MAX_DEPTH_CAP);
    if (n->init < 0 || n->init > 2) return fail("bad init mode");
    return 0;
}

static int ensure_sampler_buffers(epx_ctx *c, int chains, int nkeep) {
    if (c->s_chains == chains && c->s_nkeep == nkeep) return 0;
    const size_t K = c->K, P = c->P;
    HIPCHK(c->draws.alloc(K * chains * nkeep * P));
    HIPCHK(c->last.alloc(K * chains * P));
    HIPCHK(c->chain_stats.alloc(K * chains * ST_COUNT));
    HIPCHK(c->site_stats.alloc(K * 8));
    HIPCHK(c->team_passes.alloc(K));
    HIPCHK(hipMemset(c->team_passes, 0, K * 8));
    HIPCHK(c->seeds_d.alloc(K));
    c->carry_chains = 0;
    HIPCHK(c->carry_eps.alloc(K * chains));
    HIPCHK(c->carry_metric.alloc(K * P));
    {
        std::vector<double> neg(K * chains, -1.0);       // no history yet
        HIPCHK(hipMemcpy(c->carry_eps, neg.data(), neg.size() * 8, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemset(c->last, 0, K * chains * P * 8));
    HIPCHK(hipMemset(c->chain_stats, 0, K * chains * ST_COUNT * 8));
    c->s_chains = chains; c->s_nkeep = nkeep; c->has_last = 0;
    return 0;
}

static int pad_dp(int D) { return D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : -1; }

static bool duo_layout(int layout) { return layout == 5 || layout == 6 || layout == 7; }

// The environment switches of a sampling call, read once per call
struct SamplerEnv {
    bool piece_grid;          // EPX_PIECE_GRID: a pieced launch runs one workgroup per piece instead of looping ones (A/B)
    int piece_wait_s;         // EPX_PIECE_WAIT_S: seconds a workgroup of a pieced launch looks for a site
    int yield_cycles;         // EPX_YIELD: the row team's yield budget (layout 7; A/B: 0 turns it off)
    bool no_lean;             // EPX_NO_LEAN: layout 7 with the full chain rule in every round (diagnostic)
    bool test_fail_ckpt;      // EPX_TEST_FAIL_CKPT: the checkpoint records of a pieced launch count as refused (test hook)
    bool piece_loop;          // EPX_PIECE_LOOP: diagnostic build only, a pieced launch keeps its looping workgroups
};

static SamplerEnv sampler_env() {
    const auto num = [](const char *name, int dflt) { const char *s = getenv(name); return s ? atoi(s) : dflt; };
    SamplerEnv e;
    e.piece_grid = getenv("EPX_PIECE_GRID") != nullptr;
    const int wait_s = num("EPX_PIECE_WAIT_S", 0);
    e.piece_wait_s = wait_s > 0 ? wait_s : EPX_PIECE_WAIT_S;
    e.yield_cycles = num("EPX_YIELD", EPX_YIELD_DEFAULT);
    e.no_lean = getenv("EPX_NO_LEAN") != nullptr;
    e.test_fail_ckpt = getenv("EPX_TEST_FAIL_CKPT") != nullptr;
    e.piece_loop = getenv("EPX_PIECE_LOOP") != nullptr;
    return e;
}

// What the shape and the request decide about a sampler launch
struct SamplerPlan {
    int layout, wpc, dp, nv;
    bool spins;               // the kernel's waves hand off through spins that can give up (NutsArgs::err)
    NutsArgs a;               // every field but the arrays (bind_sampler) and the form of the launch (run_sampler)
};

// layout: 1 = one block per site (wave = chain, X resident in LDS), 2 = one block per (site, chain) with 4 cooperating
// waves, 3 = streaming (chains in lock step, X through an LDS tile), 4 = lock step with the rows resident, 5 / 6 / 7 =
// row waves + state waves (nuts_duo.hip).  No HIP call, no allocation, no change to the context.
static int plan_sampler(const epx_ctx &c, int count, const epx_sampler_opts &o, const SamplerEnv &env, SamplerPlan *p) {
    NutsArgs &a = p->a;
    memset(&a, 0, sizeof a);
    a.dyn_tail_div = 1;                                 // (a divisor: never 0, also for launches that do not come from the piece queue)
    a.model = c.model; a.D = c.D; a.d = c.d; a.P = c.P;
    a.gauss = c.gauss;
    a.chains = o.chains; a.iter = o.iter; a.warmup = o.warmup; a.thin = o.thin; a.nkeep = (o.iter - o.warmup + o.thin - 1) / o.thin;
    a.max_depth = o.max_depth; a.init_mode = o.init;
    a.ngmax = c.ng_max; a.ntmax = c.nt_max;
    const int no_spec = o.reserved & 1;           // flag: bookkeeping on the gradient waves (A/B and tests)
    const int nv = (c.P + 63) / 64;
    int dp = pad_dp(c.D);
    p->nv = nv;
    p->spins = false;
    // resident layouts: enough sites to fill the 256 CUs -> one block per site, else one block
    // per (site, chain) with 4 cooperating waves
    int layout = o.layout;
    // one workgroup per (site, chain) schedules chain by chain (no waiting for the slowest of a site's
    // chains) and has the shorter leapfrog; one workgroup per site packs 4 chains on a CU.  Measured
    // cross-over at the C2 site size, where two layout-2 workgroups share a CU (scripts/tick_occupancy.py:
    // layout 2 ahead by 24 % at 192 sites, 5 % at 256, behind by 4 % at 512); 192 when only one fits.
    bool many = count >= 192;
    if (layout == 0 && !c.multi && dp > 0 && nv <= 2) {
        NutsArgs t = a;
        t.cpb = 1;
        const size_t lds2 = nuts_lds_layout(t, 4, dp, c.n_max);
        if (2 * lds2 <= LDS_CAP) many = count >= 320;
    }
    // layout 4: one block per site, chains in lock step, rows resident in LDS, MFMA products: the
    // home of multi-group sites with small D (measured 1.05-1.4x faster than streaming them);
    // for single-group sites layout 1 is still faster at the C3 site size (132 vs 157 ms per
    // launch), so it is chosen on request only
    bool lock = false;
    // several groups per site: one workgroup per chain, the four gradient waves share the
    // site's groups (nuts_gradient_groups.inc); needs rows, Omega, tree stack and mailbox in LDS
    // (an attempt that does not fit leaves its LDS offsets in `a`: the forms below lay out their own)
    bool grp = false;
    if (c.multi && dp > 0 && nv <= 2 && !no_spec &&
        (layout == 2 || layout == 0)) {       // measured ahead of the lock-step layouts from 32 to 1024 sites (scripts/ab_kj.py)
        a.grp = 1; a.cpb = 1;
        const size_t lds = nuts_lds_layout(a, 4, dp, c.n_max);
        if (lds <= LDS_CAP && a.om_in_lds && a.stack_in_lds && a.off_spec > 0) grp = true;
        else a.grp = 0;
    }
    if (grp) {
        a.no_spec = 0;
        p->wpc = 4; p->dp = dp; p->layout = 2;
        return 0;
    }
    // (Gaussian-likelihood sites that do not fit the resident forms above are streamed: layout 3)
    if (layout == 2 && c.multi) layout = 0;
    if ((layout == 4 || (layout == 0 && c.multi)) && c.D <= 32 && nv <= 7 && !c.gauss) {
        const int dpl = c.D <= 16 ? 16 : 32;
        size_t lds = nuts_stream_lds_bytes(nv, dpl, c.d, c.ng_max, c.nt_max, c.n_max, 0);
        if (lds <= LDS_CAP) {
            lock = true; layout = 4; dp = dpl;
            a.cpb = 4; a.n_max = c.n_max; a.stack_in_lds = 0; a.om_in_lds = 0;
            const size_t om = (size_t)c.d * c.d * 8;
            if (lds + om <= LDS_CAP) { a.om_in_lds = 1; lds += om; }       // small sites: Omega next to the rows
            a.lds_bytes = (int)lds;
        }
    }
    if (layout == 4 && !lock) layout = 0;
    // layouts 5 / 6 (nuts_duo.hip): row waves + a state wave per chain, LDS hand-offs.  5 = one workgroup per
    // site (up to 4 chains), the default for batches that fill the chip; 6 = one workgroup per chain with 4 row waves
    // Few sites, models with per-coefficient scales (m4b / m5b): layout 6 by default -- its state wave runs from the
    // "view" alone (nuts_duo.hip), 374 against 413 ms per C2 iteration of layout 2; the other models stay on layout 2
    // (only when every chain has a CU of its own: the regime where a launch is as long as its slowest chain)
    const bool auto6 = layout == 0 && !many && c.model >= EPX_M4B_SG && count * o.chains <= c.n_cu;
    if (!lock && !c.multi && !c.gauss && dp > 0 && nv <= 2 && !no_spec &&
        (layout == 5 || layout == 6 || layout == 7 || (layout == 0 && many) || auto6)) {
        // layout 7: the row TEAM of nuts_duo.hip -- four row waves serve the four chains of a site in lock step on the
        // matrix pipe, the state waves are layout 5's; the default for batches that fill the chip since round 3 (layout 5
        // when the TEAM form does not fit the LDS: it pads the rows to whole 16-row tiles)
        int cand[2], ncand = 0;
        if (layout == 6 || auto6) cand[ncand++] = 6;
        else if (layout == 5) cand[ncand++] = 5;
        else { cand[ncand++] = 7; cand[ncand++] = 5; }         // (a request for 7 that does not fit is served by 5)
        for (int ic = 0; ic < ncand; ++ic) {
            const bool six = cand[ic] == 6, seven = cand[ic] == 7;
            const int cpb = six ? 1 : 4, rw = six ? 2 : (seven ? 4 : 1);
            NutsArgs t = a;
            const size_t lds = nuts_duo_lds_layout(t, cpb, rw, dp, c.n_max);
            // (layout 6: one chain per workgroup, the bookkeeping wave's stack lives in LDS or the layout is not used)
            const bool fits = nuts_duo_has(cpb, rw, dp, nv) && lds <= LDS_CAP &&
                              (seven ? (c.n_max + 63) / 64 <= 32 : (c.n_max + 64 * rw - 1) / (64 * rw) <= 64) &&
                              (!six || t.stack_in_lds);
            if (!fits) continue;
            a = t;
            a.stack_stride = nuts_resident_chain_doubles(nv, o.max_depth);
            a.no_spec = seven && env.no_lean;                   // (diagnostic: layout 7 with the full chain rule in every round)
            a.yield_cycles = seven ? env.yield_cycles : 0;
            p->wpc = rw; p->dp = dp; p->layout = cand[ic]; p->spins = true;
            return 0;
        }
        if (layout == 5 || layout == 6 || layout == 7) layout = 0;
    }
    if (layout == 0) layout = many ? 1 : 2;
    int wpc = 1;
    bool resident = !lock && dp > 0 && nv <= 2 && layout != 3 && !c.multi;      // several groups per site: layouts 3 / 4 only
    if (resident) {
        if (layout == 1) { wpc = 1; a.cpb = o.chains < 4 ? o.chains : 4; }
        else { wpc = 4; a.cpb = 1; }
        const size_t lds = nuts_lds_layout(a, wpc, dp, c.n_max);
        if (lds > LDS_CAP) resident = false;
    }
    if (c.gauss) {
        // Gaussian-likelihood family: the resident kernels are built for their everything-in-LDS forms; any other
        // shape (rows beyond the LDS, D > 32, several groups with many coordinates) is streamed (layout 3)
        const bool ok = resident && a.om_in_lds && (wpc == 1 || (a.stack_in_lds && a.off_spec > 0 && !no_spec));
        if (!ok) resident = false;
    }
    if (!resident && !lock) {
        // rows (or parameters) do not fit the resident kernel: stream X through an LDS tile
        layout = 3;
        if (c.D > 128) return fail("D = %d > 128 is not supported by the streaming sampler", c.D);
        if (nv > 7) return fail("P = %d > 448 sampled coordinates not supported", c.P);
        dp = c.D <= 64 ? 64 : 128;
        a.cpb = 4; wpc = 1;
        a.stack_in_lds = 0; a.om_in_lds = 0;
        a.lds_bytes = (int)nuts_stream_lds_bytes(nv, dp, c.d, c.ng_max, c.nt_max, 0, c.gauss);
        a.off_piece = a.lds_bytes; a.lds_bytes += 16;       // (site, first transition) of a pieced launch's workgroup
        p->spins = true;
        if ((size_t)a.lds_bytes > LDS_CAP) return fail("streaming sampler needs %d B of LDS", a.lds_bytes);
    }
    if (!a.stack_in_lds)
        a.stack_stride = layout >= 3 ? nuts_stream_chain_doubles(nv, o.max_depth) : nuts_resident_chain_doubles(nv, o.max_depth);
    a.no_spec = no_spec;
    p->wpc = wpc; p->dp = dp; p->layout = layout;
    return 0;
}

// The context's arrays into the arguments of a planned launch.  Called once every buffer of the call has its size:
// nothing is re-allocated behind it.
static NutsArgs bind_sampler(const epx_ctx &c, int k0, const SamplerPlan &p) {
    NutsArgs a = p.a;
    a.k0 = k0;
    a.k_lim = c.k_lim_d; a.X = c.X; a.y = c.y; a.y32 = c.y32; a.yd = c.yd; a.cav_Om = c.cav_Om; a.cav_mu = c.cav_mu;
    a.site_g0 = c.site_g0_d; a.g_lim = c.g_lim_d;
    if (p.spins) a.err = c.err_flag;
    if (a.stack_stride) a.stack = c.stack;                              // (tree stack + cold store in global memory)
    return a;
}

static int launch_sampler(const SamplerPlan &p, const NutsArgs &a, int count, hipStream_t stream) {
    if (duo_layout(p.layout)) return launch_nuts_duo(a, count, a.cpb, a.duo_rw, p.dp, p.nv, stream);
    if (p.layout >= 3) return launch_nuts_stream(a, count, p.dp, p.nv, stream);
    return launch_nuts(a, count, p.wpc, p.dp, p.nv, stream);
}

// Piece queue (epx_set_piece_queue): one workgroup per piece, sites claimed by largest remaining predicted work.  The
// test hook epx_sample_piece runs ONE transition per site from injected checkpoint records the same way.
struct PieceQueue {
    bool on = false;
    int len = 0;              // nominal transitions of a piece
    int tail_div = 1;         // the pieces behind 3/4 of a site's run are len / tail_div long (epx_pieces.h)
    int nb_site = 0;          // piece boundaries (checkpoint records) per site
    int nwg = 0;              // workgroups: at most one per piece (looping ones: the launcher cuts it to what the device holds)
    bool looping = false;     // the workgroups loop over claims instead of running one piece each
    size_t stack_elems = 0, ckpt_elems = 0;
};

static PieceQueue plan_queue(const epx_ctx &c, int k0, int count, const epx_sampler_opts &o, const SamplerPlan &p,
                             const SamplerEnv &env, bool fixed_steps) {
    PieceQueue q;
    const bool hook = c.hook_t0 > 0;
    q.on = (c.dyn_len > 0 || hook) && (p.layout == 5 || p.layout == 7 || p.layout == 3) && k0 == 0 && count == c.K &&
           o.chains <= p.a.cpb && !fixed_steps && (o.layout == 0 || o.layout == p.layout);
    if (!q.on) return q;
    q.len = hook ? 1 : c.dyn_len;
    // Shorter pieces behind 3/4 of a site's run (epx_pieces.h): a quarter of the nominal length for the STREAMING sampler
    // (layout 3; same-box A/B at the C5 shard: +0.7 %, profiles/r05_piece_tail_ab.txt), one length throughout for the resident
    // layouts -- there a piece start re-stages the site's 128 KB of rows, the A/B showed no gain (546.6 / 545.9 / 545.6 /
    // 545.8 site-updates/s) and the extra pieces cost 7 GB of HBM traffic per C3 launch.
    q.tail_div = p.layout == 3 ? 4 : 1;
    const int np = piece_boundaries(o.iter, q.len, q.tail_div);     // (nominal pieces, then shorter ones behind 3/4 of the run)
    const size_t pieces = (size_t)count * np;
    q.nb_site = np + 1;
    // (the hook: `count` workgroups of the one-piece-per-workgroup form claim one site each and run ONE transition)
    q.nwg = hook ? count : (int)pieces;
    q.looping = !env.piece_grid && !hook;
#ifdef EPX_STAMPS
    if (!env.piece_loop) q.looping = false;     // (the diagnostic build's records are per workgroup: one piece each unless asked otherwise)
#endif
    // A pieced launch keeps tree stack + cold store per WORKGROUP (1 GB at the C5 shard; 4 GB with one region per piece)
    // and a checkpoint record per piece boundary.  (Looping workgroups keep theirs per RESIDENT workgroup: never more than
    // 8 per CU; with one workgroup per piece, EPX_PIECE_GRID, every piece has its own.)
    const size_t regions = (q.looping && pieces > (size_t)c.n_cu * 8) ? (size_t)c.n_cu * 8 : pieces;
    q.stack_elems = regions * o.chains * p.a.stack_stride;
    q.ckpt_elems = (size_t)count * q.nb_site * o.chains * piece_record_doubles(p.nv);
    return q;
}

// the queue's words and checkpoint records into the launch (behind the allocations)
static int bind_queue(epx_ctx *c, const PieceQueue &q, int count, const epx_sampler_opts &o, const SamplerEnv &env, int nv,
                      NutsArgs *a) {
    const bool hook = c->hook_t0 > 0;
    HIPCHK(hipMemsetAsync(c->dyn_words, 0, 2 * (size_t)count * sizeof(int), c->stream));      // (stream-ordered in front of the launch)
    a->dyn_prog = c->dyn_words; a->dyn_busy = c->dyn_words + count;
    a->dyn_rate = (c->dyn_has_rate && !hook) ? c->dyn_rate.p : nullptr;
    a->dyn_len = q.len; a->dyn_count = count; a->dyn_hook = hook;
    a->dyn_wait_s = env.piece_wait_s;
    a->dyn_nb = q.nb_site; a->dyn_tail_div = q.tail_div;
    a->seg_nwg = q.nwg; a->persist = q.looping;
    a->ckpt = c->ckpt;                                   // (one record per piece boundary of a site)
    a->order = nullptr;
    if (hook) {
        // every site stands at transition t0 with the caller's records at that boundary; the piece leaves the record of
        // boundary t0 + 1
        std::vector<int> prog((size_t)count, 2 * c->hook_t0);
        HIPCHK(hipStreamSynchronize(c->stream));        // (the memset above is stream-ordered, this copy is not)
        HIPCHK(hipMemcpy(c->dyn_words, prog.data(), (size_t)count * sizeof(int), hipMemcpyHostToDevice));
        const size_t rec = piece_record_doubles(nv);
        for (int k = 0; k < count; ++k)
            HIPCHK(hipMemcpy(c->ckpt + (((size_t)k * q.nb_site + c->hook_t0) * o.chains) * rec,
                             c->hook_in + (size_t)k * o.chains * rec, (size_t)o.chains * rec * 8, hipMemcpyHostToDevice));
    }
    c->last_segments = -((o.iter + q.len - 1) / q.len);      // (negative: pieces per site of a queued launch, at the nominal length)
    return 0;
}

// Split launch (epx_set_site_split): the leading sites of the order -- the ones expected to need the most leapfrogs --
// run one workgroup per chain (layout 2, shorter leapfrog) on a second queue while the rest run one workgroup per site
// (layout 1, more chains per CU).  The launch ends with its slowest chain; this takes that chain at the faster tick.
// Returns the number of lead sites (0: no split), -1 on an error.
static int plan_split(const epx_ctx &c, int count, const epx_sampler_opts &o, const SamplerEnv &env, const SamplerPlan &p,
                      SamplerPlan *lead) {
    if (o.layout != 0 || !(p.layout == 1 || p.layout == 5 || p.layout == 7) || c.split_n <= 0) return 0;
    int n_lead = c.split_n < count ? c.split_n : count - 1;
    const int cap = c.n_cu / (2 * o.chains);          // at most half of the CUs for the lead sites
    if (n_lead > cap) n_lead = cap;
    if (n_lead <= 0) return 0;
    epx_sampler_opts o2 = o;
    o2.layout = 2;
    if (plan_sampler(c, n_lead, o2, env, lead)) return -1;
    return lead->layout == 2 ? n_lead : 0;
}

static int run_sampler(epx_ctx *c, int k0, int count, const int64_t *seeds, const epx_sampler_opts &o,
                       double *elapsed_ms, const double *eps_dev = nullptr,
                       const double *inv_e_dev = nullptr, int t_offset = 0) {
    const int nkeep = (o.iter - o.warmup + o.thin - 1) / o.thin;
    if (ensure_sampler_buffers(c, o.chains, nkeep)) return -1;
    if (o.init == EPX_INIT_PREV && !c->has_last) return fail("init=PREV before any sampling call");
    const SamplerEnv env = sampler_env();
    const bool hook = c->hook_t0 > 0;          // epx_sample_piece
    const int *order = (c->order_d && c->order_n == count && k0 == 0) ? c->order_d.p : nullptr;

    // 1. plan the launch, and the lead part of a split launch (it runs when the launch is not pieced)
    SamplerPlan p, lead;
    if (plan_sampler(*c, count, o, env, &p)) return -1;
    c->last_segments = 0;
    c->trace_chains = 0;
#ifdef EPX_STAMPS
    const bool may_split = false;       // (the diagnostic build's records are per workgroup of ONE launch)
#else
    const bool may_split = order && !eps_dev;
#endif
    int n_lead = 0;
    if (may_split && (n_lead = plan_split(*c, count, o, env, p, &lead)) < 0) return -1;
    // 2. the piece queue
    PieceQueue q = plan_queue(*c, k0, count, o, p, env, eps_dev != nullptr);
    if (hook && (!q.on || c->hook_t0 >= o.iter))
        return fail("epx_sample_piece: needs a piece-capable layout (5, 7, 3; got %d) over all sites and 0 < t0 < iter", p.layout);
    // 3. sizes.  The tree stack is indexed by site of the batch: the two launches of a split share it
    const size_t stride = std::max(p.a.stack_stride, n_lead ? lead.a.stack_stride : (size_t)0);
    const size_t stack_elems = (size_t)count * o.chains * stride;
    const int ts = (c->trace_sites > 0 && !eps_dev) ? std::min(c->trace_sites, count) : 0;     // (test hook epx_set_trace)
    const size_t trace_elems = (size_t)ts * o.chains * o.iter * (size_t)(8 + c->P);
    // 4. grow.  If the device cannot give the pieced launch its memory, the launch runs unpieced -- same draws, one
    // workgroup per site -- instead of failing the sampling call (EPX_TEST_FAIL_CKPT: the test hook of that fallback)
    if (q.on && !(c->stack.try_grow(std::max(stack_elems, q.stack_elems)) &&
                  (env.test_fail_ckpt ? c->ckpt.n >= q.ckpt_elems : c->ckpt.try_grow(q.ckpt_elems))))
        q.on = false;
    // (the hook has no unpieced form: if the records could not be had, the call fails instead of running a whole update
    // and copying out of a checkpoint buffer that is missing or too small)
    if (hook && !q.on) return fail("epx_sample_piece: the checkpoint records / tree stacks of the pieced launch could not be allocated");
    if (q.on) n_lead = 0;
    HIPCHK(c->stack.grow(stack_elems));
    if (c->reuse_on) {      // epx_set_draw_reuse: room for the cavities this call samples against
        HIPCHK(c->drawn_Om.grow((size_t)c->K * c->d * c->d));
        HIPCHK(c->drawn_mu.grow((size_t)c->K * c->d));
    }
    if (q.on) HIPCHK(c->dyn_words.grow(2 * (size_t)c->K));
    if (ts) HIPCHK(c->trace.grow(trace_elems));
#ifdef EPX_STAMPS
    // (per workgroup three records of 8 sums: the roles' shares, then the phases of the row team's pass; behind them two
    // records of the first diagnostic form and six of histograms.  A pieced launch: one workgroup per piece)
    const int nblk = q.on ? q.nwg : count * ((o.chains + p.a.cpb - 1) / p.a.cpb);
    const size_t stamp_recs = (size_t)3 * nblk + 8;
    HIPCHK(c->stamps.grow(stamp_recs * 8));
#endif
    // 5. bind
    const auto bind = [&](const SamplerPlan &pl) {
        NutsArgs b = bind_sampler(*c, k0, pl);
        b.seeds = c->seeds_d; b.draws = c->draws; b.last = c->last; b.chain_stats = c->chain_stats;
        b.team_passes = c->team_passes;
        b.eps_in = eps_dev; b.inv_e_in = inv_e_dev; b.t_offset = t_offset;
        if ((o.reserved & 2) && !eps_dev) { b.carry_eps = c->carry_eps; b.carry_metric = c->carry_metric; }
        b.order = order;
        if (ts) { b.trace = c->trace; b.trace_sites = ts; }     // (records are keyed by the REAL site, through `order`, in both launches of a split)
        return b;
    };
    NutsArgs a = bind(p), a2;
    if (n_lead > 0) { a2 = bind(lead); a.order += n_lead; }
    c->last_split = n_lead;
    HIPCHK(hipMemsetAsync(c->team_passes + k0, 0, (size_t)count * 8, c->stream));
    if (ts) {
        HIPCHK(hipMemsetAsync(c->trace, 0, trace_elems * 8, c->stream));
        c->trace_chains = o.chains; c->trace_iter = o.iter; c->trace_last_sites = ts;
    }
    if (q.on && bind_queue(c, q, count, o, env, p.nv, &a)) return -1;
#ifdef EPX_STAMPS
    HIPCHK(hipMemset(c->stamps, 0, stamp_recs * 64));
    a.stamps = c->stamps; a.stamps_nrec = nblk;
    c->stamps_last = stamp_recs;
#endif
    // 6. launch
    HIPCHK(hipMemcpyAsync(c->seeds_d, seeds, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    int rc = 0;
    if (n_lead > 0) {
        HIPCHK(hipEventRecord(c->ev_fork, c->stream));
        HIPCHK(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
        rc = launch_sampler(lead, a2, n_lead, c->stream2);
        HIPCHK(hipEventRecord(c->ev_join, c->stream2));
    }
    if (rc == 0) rc = launch_sampler(p, a, count - n_lead, c->stream);
    if (n_lead > 0) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    if (rc != 0) return fail("NUTS kernel launch failed (%d: %s)", rc, rc > 0 ? hipGetErrorString((hipError_t)rc) : "unsupported shape");
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    c->snap_count = 0;
    if (c->reuse_on) {
        const size_t d = c->d, dd = d * d;
        HIPCHK(hipMemcpyAsync(c->drawn_Om + k0 * dd, c->cav_Om + k0 * dd, count * dd * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->drawn_mu + k0 * d, c->cav_mu + k0 * d, count * d * 8, hipMemcpyDeviceToDevice, c->stream));
        c->snap_k0 = k0; c->snap_count = count;
    }
    // 7. epilogue: site statistics, carry history, the hand-off error flag, the hook's records, the time
    RhatArgs ra;
    ra.k0 = k0; ra.chains = o.chains; ra.nkeep = nkeep; ra.P = c->P;
    ra.site_g0 = c->site_g0_d; ra.d = c->d; ra.pg = c->pg;
    ra.draws = c->draws; ra.chain_stats = c->chain_stats; ra.site_stats = c->site_stats;
    hipLaunchKernelGGL(k_site_stats, dim3(count), dim3(128), 0, c->stream, ra);
    HIPCHK(hipGetLastError());
    if (!eps_dev) {
        // history for `adapt = carry` (cheap: one pass over the kept draws); written after every real sampling call
        CarryArgs ca;
        ca.k0 = k0; ca.chains = o.chains; ca.nkeep = nkeep; ca.P = c->P;
        ca.draws = c->draws; ca.chain_stats = c->chain_stats; ca.carry_eps = c->carry_eps; ca.carry_metric = c->carry_metric;
        hipLaunchKernelGGL(k_carry_update, dim3(count), dim3(128), 0, c->stream, ca);
        HIPCHK(hipGetLastError());
        c->carry_chains = o.chains;
    }
    c->has_last = 1;
    c->last_layout = p.layout;
    c->nsamp = o.chains * nkeep;
    c->drawn_k0 = k0; c->drawn_count = count;       // the sites whose draws this call leaves behind (epx_named_moments)
    int herr = 0;
    {
        // (no return between a queued copy into this frame and the synchronisation)
        hipError_t e = hipSuccess;
        if (duo_layout(p.layout) || q.on) e = hipMemcpyAsync(&herr, c->err_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream);
        const hipError_t es = hipStreamSynchronize(c->stream);
        HIPCHK(e);
        HIPCHK(es);
    }
    if (hook && c->hook_out && !herr) {
        const size_t rec = piece_record_doubles(p.nv);
        for (int k = 0; k < count; ++k)
            HIPCHK(hipMemcpy(c->hook_out + (size_t)k * o.chains * rec,
                             c->ckpt + (((size_t)k * q.nb_site + c->hook_t0 + 1) * o.chains) * rec, (size_t)o.chains * rec * 8, hipMemcpyDeviceToHost));
    }
    if (herr) {
        HIPCHK(hipMemset(c->err_flag, 0, sizeof(int)));
        c->drawn_count = 0; c->snap_count = 0;
        return fail("sampler: a hand-off between the waves of a chain timed out (code %d); the draws of this call are void", herr);
    }
    if (elapsed_ms) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        *elapsed_ms = ms;
    }
    return 0;
}

// what the moment stage refuses of a call's draws, in front of any copy of them
static int check_moments(const epx_ctx *c, int S, int prec_estim) {
    if (prec_estim != EPX_PREC_SAMPLE && prec_estim != EPX_PREC_OLSE) return fail("bad prec_estim %d", prec_estim);
    if (S < c->d) return fail("fewer draws (%d) than dimensions (%d)", S, c->d);   // method.py:427 raises ValueError
    return 0;
}

static int launch_moments(epx_ctx *c, int k0, int count, const double *draws, long site0,
                          long stride_site, long stride_s, long stride_i, int S, int prec_estim) {
    MomentArgs a;
    a.k0 = k0; a.S = S; a.prec_estim = prec_estim;
    a.draws = draws; a.draws_site0 = site0; a.stride_site = stride_site; a.stride_s = stride_s; a.stride_i = stride_i;
    a.Q = c->Q; a.r = c->r; a.dQi = c->dQi; a.dri = c->dri;
    a.tilt_mean = c->tilt_mean; a.tilt_scatter = c->tilt_scatter; a.flags = c->flags;
    return launch_dense(k_moments, count, c->stream, c->dense_ws, c->d, count, a);
}

int epx_sample_batch(epx_ctx *c, int k0, int count, const int64_t *seeds, const epx_sampler_opts *opts,
                     double *stats, double *elapsed_ms) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    epx_sampler_opts o;
    if (norm_opts(opts, &o)) return -1;
    if (run_sampler(c, k0, count, seeds, o, elapsed_ms)) return -1;
    if (stats) HIPCHK(hipMemcpy(stats, c->site_stats, (size_t)count * 8 * 8, hipMemcpyDeviceToHost));
    return 0;
}

int epx_sample_piece(epx_ctx *c, const int64_t *seeds, const epx_sampler_opts *opts, int t0,
                     const double *records_in, double *records_out) {
    CTX(c);
    epx_sampler_opts o;
    if (norm_opts(opts, &o)) return -1;
    if (t0 <= 0 || !records_in) return fail("epx_sample_piece: t0 > 0 and the records of that boundary are required");
    c->hook_t0 = t0; c->hook_in = records_in; c->hook_out = records_out;
    const int rc = run_sampler(c, 0, c->K, seeds, o, nullptr);
    c->hook_t0 = 0; c->hook_in = nullptr; c->hook_out = nullptr;
    return rc ? -1 : 0;
}

int epx_tilted_batch(epx_ctx *c, int k0, int count, const int64_t *seeds, const epx_sampler_opts *opts,
                     int prec_estim, uint8_t *posdef, double *stats, double *elapsed_ms) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    epx_sampler_opts o;
    if (norm_opts(opts, &o)) return -1;
    if (run_sampler(c, k0, count, seeds, o, elapsed_ms)) return -1;
    const int nkeep = c->s_nkeep;
    if (check_moments(c, o.chains * nkeep, prec_estim)) return -1;
    // native draw layout: (site, chain, keep, P) -> draw s = chain*nkeep + keep is contiguous
    if (launch_moments(c, k0, count, c->draws, k0, (long)o.chains * nkeep * c->P, c->P, 1,
                       o.chains * nkeep, prec_estim)) return -1;
    if (fetch_flags(c, k0, count, posdef)) return -1;
    if (stats) HIPCHK(hipMemcpy(stats, c->site_stats, (size_t)count * 8 * 8, hipMemcpyDeviceToHost));
    return 0;
}

int epx_moments_batch(epx_ctx *c, int k0, int count, const double *samples, int S, int prec_estim,
                      uint8_t *posdef) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    if (check_moments(c, S, prec_estim)) return -1;
    const size_t need = (size_t)count * S * c->d;
    HIPCHK(c->inj.grow(need));
    HIPCHK(hipMemcpy(c->inj, samples, need * 8, hipMemcpyHostToDevice));
    // (S, d) F-order per site: element (s, i) at i*S + s
    if (launch_moments(c, k0, count, c->inj, 0, (long)S * c->d, 1, S, S, prec_estim)) return -1;
    if (fetch_flags(c, k0, count, posdef)) return -1;
    c->nsamp = S;
    return 0;
}

int epx_set_draw_reuse(epx_ctx *c, int on) {
    if (!c) return fail("null context");
    c->reuse_on = on ? 1 : 0;
    if (!on) c->snap_count = 0;
    return 0;
}

int epx_reweight_batch(epx_ctx *c, int k0, int count, int prec_estim, const double *theta, int S,
                       const double *Om_old, const double *mu_old, uint8_t *posdef, double *out, double *elapsed_ms) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    if (theta && (!Om_old || !mu_old)) return fail("epx_reweight_batch: draws of the caller need Om_old and mu_old, the cavity they were sampled against");
    DrawSource src;
    if (draw_source(c, "epx_reweight_batch", k0, count, theta, S, nullptr, &src)) return -1;
    S = src.S;
    if (check_moments(c, S, prec_estim)) return -1;
    // the LDS plan: [work matrices and vectors (DensePlan), when they fit beside the rest | -lr (Sp) | w (Sp) | PSIS scratch of
    // one row | the tail's draw indices (M ints)]
    const size_t d = c->d;
    const DensePlan p(c->d);
    ReweightArgs a;
    a.M = psis_tail_length(S); a.mfit = psis_fit_points(a.M); a.Sp = (S + 1) / 2 * 2;
    const size_t extra = 2 * (size_t)a.Sp + psis_scratch_doubles(a.M) + psis_tail_pad(a.M) / 2 + 1;
    if (a.mfit > PSIS_FIT_MAX || extra * 8 + 1024 > LDS_CAP)
        return fail("epx_reweight_batch: S = %d draws: the ratios and weights of a site do not fit the LDS", S);
    const bool in_lds = (p.slot + extra) * 8 + 1024 <= LDS_CAP;
    if (!theta && (!c->drawn_Om || k0 < c->snap_k0 || k0 + count > c->snap_k0 + c->snap_count))
        return fail("epx_reweight_batch: no record of the cavity the draws of sites [%d,%d) were sampled against: switch "
                    "epx_set_draw_reuse on before the sampling call", k0, k0 + count);
    HIPCHK(c->dense_ws.grow(in_lds ? 0 : p.slot * (size_t)count));
    HIPCHK(c->rw_out.grow((size_t)count * EPX_RW_COUNT));
    if (theta) HIPCHK(c->rw_old.grow((size_t)count * (d * d + d)));
    a.extra_at = in_lds ? (int)p.slot : 0;
    const size_t lds = ((in_lds ? p.slot : 0) + extra) * 8;
    if (set_lds(k_reweight, lds)) return -1;
    MomentArgs &m = a.m;
    m.k0 = k0; m.d = c->d; m.ld = p.ld; m.S = S; m.prec_estim = prec_estim;
    m.ws.use_lds = in_lds; m.ws.global = in_lds ? nullptr : c->dense_ws.p;
    m.draws_site0 = 0; m.stride_site = (long)S * c->P; m.stride_s = c->P; m.stride_i = 1;
    m.Q = c->Q; m.r = c->r; m.dQi = c->dQi; m.dri = c->dri;
    m.tilt_mean = c->tilt_mean; m.tilt_scatter = c->tilt_scatter; m.flags = c->flags;
    a.Om_new = c->cav_Om + k0 * d * d; a.mu_new = c->cav_mu + k0 * d;
    a.rec = c->rw_out;
    StreamSync sync{c->stream};
    if (upload_draws(c, src, &m.draws)) return -1;
    if (theta) {
        HIPCHK(hipMemcpyAsync(c->rw_old, Om_old, count * d * d * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->rw_old + count * d * d, mu_old, count * d * 8, hipMemcpyHostToDevice, c->stream));
        a.Om_old = c->rw_old; a.mu_old = c->rw_old + count * d * d;
    } else {
        a.Om_old = c->drawn_Om + k0 * d * d; a.mu_old = c->drawn_mu + k0 * d;
    }
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    hipLaunchKernelGGL(k_reweight, dim3(count), dim3(256), lds, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    if (posdef) HIPCHK(hipMemcpyAsync(posdef, c->flags + k0, count, hipMemcpyDeviceToHost, c->stream));
    if (out) HIPCHK(hipMemcpyAsync(out, c->rw_out, (size_t)count * EPX_RW_COUNT * 8, hipMemcpyDeviceToHost, c->stream));
    if (sync.finish()) return -1;
    c->nsamp = S;
    if (elapsed_ms) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        *elapsed_ms = ms;
    }
    return 0;
}

int epx_get_tilted(epx_ctx *c, int k, double *Mat, double *vec, int *nsamp) {
    CTX(c);
    if (check_range(c, k, 1)) return -1;
    if (copy_pair(c, c->tilt_scatter, c->tilt_mean, k, 1, Mat, vec)) return -1;
    if (nsamp) *nsamp = c->nsamp;
    return 0;
}

int epx_num_draws(epx_ctx *c, int *S) {
    if (!c) return fail("null context");
    *S = c->s_chains * c->s_nkeep;
    return 0;
}

int epx_get_draws(epx_ctx *c, int k, int all_params, double *out) {
    CTX(c);
    if (check_range(c, k, 1)) return -1;
    if (!c->draws) return fail("no draws yet");
    const size_t S = (size_t)c->s_chains * c->s_nkeep, P = c->P;
    std::vector<double> tmp(S * P);
    HIPCHK(hipMemcpy(tmp.data(), c->draws + (size_t)k * S * P, S * P * 8, hipMemcpyDeviceToHost));
    const size_t ncol = all_params ? P : (size_t)c->d;
    for (size_t j = 0; j < ncol; ++j)
        for (size_t s = 0; s < S; ++s) out[j * S + s] = tmp[s * P + j];      // (S, ncol) F-order
    return 0;
}

int epx_nuts_transitions(epx_ctx *c, int k0, int count, const int64_t *seeds, int chains, int nt,
                         int t_offset, int layout, const double *q0, const double *eps,
                         const double *inv_e, double *q_out, double *chain_stats) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    epx_sampler_opts o;
    memset(&o, 0, sizeof o);
    o.chains = chains; o.iter = nt; o.warmup = 0; o.thin = 1; o.init = EPX_INIT_PREV; o.max_depth = 10;
    o.layout = layout;
    epx_sampler_opts on;
    if (norm_opts(&o, &on)) return -1;
    if (ensure_sampler_buffers(c, chains, nt)) return -1;
    const size_t P = c->P, nc = (size_t)count * chains;
    HIPCHK(hipMemcpy(c->last + (size_t)k0 * chains * P, q0, nc * P * 8, hipMemcpyHostToDevice));
    c->has_last = 1;
    DevBuf<double> eps_d, inv_d;
    HIPCHK(eps_d.alloc(nc));
    HIPCHK(inv_d.alloc(nc * P));
    HIPCHK(hipMemcpy(eps_d, eps, nc * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(inv_d, inv_e, nc * P * 8, hipMemcpyHostToDevice));
    if (run_sampler(c, k0, count, seeds, on, nullptr, eps_d, inv_d, t_offset)) return -1;
    if (q_out) HIPCHK(hipMemcpy(q_out, c->draws + (size_t)k0 * chains * nt * P, nc * nt * P * 8, hipMemcpyDeviceToHost));
    if (chain_stats) HIPCHK(hipMemcpy(chain_stats, c->chain_stats + (size_t)k0 * chains * ST_COUNT,
                                      nc * ST_COUNT * 8, hipMemcpyDeviceToHost));
    return 0;
}

#ifdef EPX_STAMPS
// diagnostic build only: cycle sums of the last sampler launch, (nblocks, 8)
extern "C" int epx_dbg_get_stamps(epx_ctx *c, unsigned long long *out, int max_blocks) {
    CTX(c);
    size_t nb = c->stamps_last < (size_t)max_blocks ? c->stamps_last : (size_t)max_blocks;
    HIPCHK(hipMemcpy(out, c->stamps, nb * 64, hipMemcpyDeviceToHost));
    return (int)nb;
}
#endif

int epx_set_site_order(epx_ctx *c, const int32_t *order, int count) {
    CTX(c);
    if (!order || count <= 0) { c->order_n = 0; return 0; }
    if (count > c->K) return fail("site order has %d entries for %d sites", count, c->K);
    std::vector<char> seen((size_t)count, 0);
    for (int i = 0; i < count; ++i) {
        if (order[i] < 0 || order[i] >= count || seen[order[i]]) return fail("site order is not a permutation of 0..%d", count - 1);
        seen[order[i]] = 1;
    }
    HIPCHK(c->order_d.grow((size_t)c->K));
    HIPCHK(hipMemcpy(c->order_d, order, (size_t)count * sizeof(int), hipMemcpyHostToDevice));
    c->order_n = count;
    return 0;
}

int epx_set_piece_queue(epx_ctx *c, int piece_len, const double *rate) {
    CTX(c);
    if (piece_len <= 0) { c->dyn_len = 0; return 0; }
    HIPCHK(c->dyn_words.grow(2 * (size_t)c->K));
    c->dyn_has_rate = rate != nullptr;
    if (rate) {
        for (int k = 0; k < c->K; ++k)
            if (!(rate[k] > 0.0) || !std::isfinite(rate[k])) return fail("predicted work of site %d is not positive", k);
        HIPCHK(c->dyn_rate.grow((size_t)c->K));
        HIPCHK(hipMemcpy(c->dyn_rate, rate, (size_t)c->K * 8, hipMemcpyHostToDevice));
    }
    c->dyn_len = piece_len;
    return 0;
}

int epx_set_trace(epx_ctx *c, int sites) {
    CTX(c);
    if (sites < 0 || sites > c->K) return fail("trace of %d sites outside 0..%d", sites, c->K);
    c->trace_sites = sites;
    return 0;
}

int epx_get_team_passes(epx_ctx *c, int k0, int count, double *out) {
    CTX(c);
    if (!out) return fail("null argument");
    if (k0 < 0 || count < 0 || k0 + count > c->K) return fail("sites %d..%d outside 0..%d", k0, k0 + count, c->K);
    if (!c->team_passes) return fail("no sampling call yet");
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, c->team_passes + k0, (size_t)count * 8, hipMemcpyDeviceToHost));
    return 0;
}

int epx_get_trace(epx_ctx *c, double *out, long long n_out) {
    CTX(c);
    if (!c->trace || c->trace_chains <= 0) return fail("no trace: epx_set_trace before the sampling call");
    const int ts = c->trace_last_sites;
    const size_t n = (size_t)ts * c->trace_chains * c->trace_iter * (size_t)(8 + c->P);
    if ((long long)n != n_out) return fail("trace has %zu doubles, the caller expects %lld", n, n_out);
    HIPCHK(hipMemcpy(out, c->trace, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

int epx_last_segments(epx_ctx *c) {
    if (!c) return fail("null context");
    return c->last_segments;
}

int epx_set_site_split(epx_ctx *c, int n_lead) {
    CTX(c);
    if (n_lead < 0 || n_lead > c->K) return fail("site split %d outside 0..%d", n_lead, c->K);
    c->split_n = n_lead;
    return 0;
}

int epx_last_split(epx_ctx *c) {
    if (!c) return fail("null context");
    return c->last_split;
}

int epx_cu_count(epx_ctx *c) {
    if (!c) return fail("null context");
    return c->n_cu;
}

int epx_last_layout(epx_ctx *c) {
    if (!c) return fail("null context");
    return c->last_layout;
}

int epx_get_chain_stats(epx_ctx *c, int k0, int count, double *out) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    if (!c->chain_stats) return fail("no sampling call yet");
    HIPCHK(hipMemcpy(out, c->chain_stats + (size_t)k0 * c->s_chains * ST_COUNT,
                     (size_t)count * c->s_chains * ST_COUNT * 8, hipMemcpyDeviceToHost));
    return 0;
}

int epx_get_adapt(epx_ctx *c, int k, double *eps, double *metric) {
    CTX(c);
    if (check_range(c, k, 1)) return -1;
    if (!c->carry_chains) return fail("no sampling call yet");
    if (eps) HIPCHK(hipMemcpy(eps, c->carry_eps + (size_t)k * c->s_chains, (size_t)c->s_chains * 8, hipMemcpyDeviceToHost));
    if (metric) HIPCHK(hipMemcpy(metric, c->carry_metric + (size_t)k * c->P, (size_t)c->P * 8, hipMemcpyDeviceToHost));
    return 0;
}

int epx_logdensity_grad(epx_ctx *c, int k, const double *theta, double *lp, double *grad) {
    return epx_logdensity_grad_layout(c, k, theta, 2, lp, grad);
}

int epx_logdensity_grad_layout(epx_ctx *c, int k, const double *theta, int layout_req, double *lp, double *grad) {
    CTX(c);
    if (check_range(c, k, 1)) return -1;
    // the sampler kernel itself evaluates the initial point and stops (NutsArgs::dbg)
    epx_sampler_opts o;
    memset(&o, 0, sizeof o);
    o.chains = 1; o.iter = 2; o.warmup = 1; o.thin = 1; o.init = EPX_INIT_PREV; o.max_depth = 10; o.layout = layout_req;
    SamplerPlan p;
    if (plan_sampler(*c, 1, o, sampler_env(), &p)) return -1;
    HIPCHK(c->stack.grow(p.a.stack_stride));           // (one site, one chain)
    NutsArgs a = bind_sampler(*c, k, p);
    const size_t P = c->P;
    HIPCHK(hipMemcpy(c->dbg + P + 1, theta, P * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(c->dbg_seed, 0, sizeof(int64_t)));
    a.seeds = c->dbg_seed;
    a.last = c->dbg + P + 1 - (size_t)k * P;      // kernel reads last[(k*chains + chain)*P], chains = 1
    a.dbg = c->dbg;
    int rc = launch_sampler(p, a, 1, c->stream);
    if (rc != 0) return fail("NUTS kernel launch failed (%d)", rc);
    c->last_layout = p.layout;
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<double> outv(P + 1);
    HIPCHK(hipMemcpy(outv.data(), c->dbg, (P + 1) * 8, hipMemcpyDeviceToHost));
    *lp = outv[0];
    memcpy(grad, outv.data() + 1, P * 8);
    return 0;
}

// ------------------------------------------------------------- global update
int epx_packed_len(epx_ctx *c, int *len) {
    if (!c) return fail("null context");
    *len = 2 * (c->d * c->d + c->d);
    return 0;
}

// Queued: `len` sums over the sites' arrays Qi, ri, dQi, dri into `out`: `partial` per slice of sites (c->partial), k_site_sums_final across them
static int queue_site_sums(epx_ctx *c, void (*partial)(SumArgs), int len, const double *Qi, const double *ri,
                           const double *dQi, const double *dri, double *out) {
    SumArgs a;
    a.K = c->K; a.d = c->d; a.len = len; a.nslice = c->nslice;
    a.Qi = Qi; a.ri = ri; a.dQi = dQi; a.dri = dri;
    a.partial = c->partial; a.out = out;
    const int nb = (len + 255) / 256;
    hipLaunchKernelGGL(partial, dim3(nb, a.nslice), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_site_sums_final, dim3(nb), dim3(256), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

int epx_site_sums(epx_ctx *c, double *packed_host, double *packed_dev) {
    CTX(c);
    const int len = 2 * (c->d * c->d + c->d);
    double *out = packed_dev ? packed_dev : c->packed;
    if (queue_site_sums(c, k_site_sums_partial, len, c->Qi, c->ri, c->dQi, c->dri, out)) return -1;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (packed_host) HIPCHK(hipMemcpy(packed_host, out, (size_t)len * 8, hipMemcpyDeviceToHost));
    return 0;
}

int epx_mix_sums(epx_ctx *c, double *out) {
    CTX(c);
    if (!c->nsamp) return fail("no tilted moments yet");
    const int len = 2 * c->d * c->d + c->d;
    if (queue_site_sums(c, k_mix_partial, len, c->tilt_scatter, c->tilt_mean, nullptr, nullptr, c->packed)) return -1;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, c->packed, (size_t)len * 8, hipMemcpyDeviceToHost));
    return 0;
}

int epx_named_len(epx_ctx *c, int k, int name, int *len) {
    if (!c) return fail("null context");
    if (!len) return fail("epx_named_len: len is required");
    if (check_range(c, k, 1)) return -1;
    const int ng = c->multi ? c->g_cnt[k] : 1;
    const int n = named_len(name, c->model, c->D, c->d, c->gauss, ng);
    if (n < 0) return fail("named parameter %d is not defined by this site model", name);
    *len = n;
    return 0;
}

int epx_named_moments(epx_ctx *c, int k0, int count, const int32_t *names, int n_names, const double *theta, int S,
                      double *mean, double *m2, int *nsamp) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    if (!mean || !m2) return fail("epx_named_moments: mean and m2 are required");
    NamedArgs a;
    DrawSource src;
    if (named_front(c, "epx_named_moments", k0, count, names, n_names, theta, S, c->ng_max, a, &src)) return -1;
    StreamSync sync{c->stream};
    if (upload_draws(c, src, &a.draws)) return -1;
    const size_t nout = (size_t)count * a.L;
    HIPCHK(c->named_out.grow(2 * nout));
    a.mean = c->named_out; a.m2 = c->named_out + nout;
    if (launch(k_named_moments, dim3(count), dim3(256), 0, c->stream, a)) return -1;
    HIPCHK(hipMemcpyAsync(mean, a.mean, nout * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(m2, a.m2, nout * 8, hipMemcpyDeviceToHost, c->stream));
    if (nsamp) *nsamp = src.S;
    return sync.finish();
}

int epx_named_order_stats(epx_ctx *c, int k0, int count, const int32_t *names, int n_names, const int64_t *ranks,
                          int n_ranks, const double *theta, int S, double *out, int *nsamp) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    if (!out) return fail("epx_named_order_stats: out is required");
    if (check_rank_count("epx_named_order_stats", ranks, n_ranks)) return -1;
    OrderArgs a;
    DrawSource src;
    if (named_front(c, "epx_named_order_stats", k0, count, names, n_names, theta, S, c->ng_max, a.nm, &src)) return -1;
    S = src.S;
    if (S > order_max_draws())
        return fail("epx_named_order_stats: S = %d draws per site, at most %d (a site's keys, padded to a power of two, are "
                    "sorted in LDS)", S, order_max_draws());
    if (fill_ranks("epx_named_order_stats", ranks, n_ranks, S, a.rank)) return -1;
    if ((long long)count * a.nm.L > 0x7fffffffLL)
        return fail("epx_named_order_stats: %d sites x %d elements in one call, at most 2^31 - 1", count, a.nm.L);
    a.n_ranks = n_ranks;
    a.npad = pow2_pad(S);
    const size_t lds = (size_t)a.npad * 8, nout = (size_t)count * a.nm.L * n_ranks;
    StreamSync sync{c->stream};
    if (upload_draws(c, src, &a.nm.draws)) return -1;
    HIPCHK(c->order_out.grow(nout));
    a.out = c->order_out;
    if (launch(k_site_order_stats, dim3((unsigned)(count * a.nm.L)), dim3(EPX_QT_THREADS), lds, c->stream, a)) return -1;
    HIPCHK(hipMemcpyAsync(out, a.out, nout * 8, hipMemcpyDeviceToHost, c->stream));
    if (nsamp) *nsamp = S;
    return sync.finish();
}

int epx_pooled_count_pass(epx_ctx *c, int k0, int count, const int32_t *names, int n_names, int shift,
                          const uint64_t *prefix, int n_targets, const double *theta, int S, long long *hist,
                          long long *n_nan, long long *n) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    if (!hist || !n_nan || !n) return fail("epx_pooled_count_pass: hist, n_nan and n are required");
    if (shift < 0 || shift > 56 || shift % 8 != 0) return fail("epx_pooled_count_pass: shift = %d, one of 56, 48, ..., 0", shift);
    if (n_targets < 1 || n_targets > EPX_QT_MAX_RANKS)
        return fail("epx_pooled_count_pass: between 1 and %d targets (got %d)", (int)EPX_QT_MAX_RANKS, n_targets);
    if (shift < 56 && !prefix) return fail("epx_pooled_count_pass: a pass below shift 56 needs the prefixes");
    // every site of the range holds the same elements: equal lengths of every name
    const int ng0 = c->multi ? c->g_cnt[k0] : 1;
    for (int i = 0; names && i < n_names && i < EPX_NM_MAX_REQ; ++i) {
        const int l0 = named_len(names[i], c->model, c->D, c->d, c->gauss, ng0);
        for (int k = k0 + 1; k < k0 + count; ++k) {
            const int lk = named_len(names[i], c->model, c->D, c->d, c->gauss, c->multi ? c->g_cnt[k] : 1);
            if (lk != l0)
                return fail("epx_pooled_count_pass: named parameter %d has %d elements at site %d and %d at site %d: a pool "
                            "needs equal lengths", (int)names[i], l0, k0, lk, k);
        }
    }
    CountArgs a;
    DrawSource src;
    // the row of the pool is sized by the sites of the RANGE (all alike), not by the context's largest site
    if (named_front(c, "epx_pooled_count_pass", k0, count, names, n_names, theta, S, ng0, a.nm, &src)) return -1;
    const size_t L = (size_t)a.nm.L, nt = (size_t)n_targets;
    a.ng = ng0; a.shift = shift; a.n_targets = n_targets;
    a.n = (long long)count * src.S;
    a.tile = EPX_QT_MAX_TILE;
    while (a.tile > 1 && (count_lds_bytes(a.tile, n_targets) > EPX_QT_COUNT_LDS || (size_t)a.tile / 2 >= L)) a.tile /= 2;
    const size_t lds = count_lds_bytes(a.tile, n_targets);
    // slabs of at least 1024 records, about 2048 workgroups in all, at most 2^20 records each (32-bit counts in LDS)
    const long long ntile = ((long long)L + a.tile - 1) / a.tile;
    long long nslab = (a.n + 1023) / 1024;
    const long long cap = 2048 / ntile > 1 ? 2048 / ntile : 1;
    if (nslab > cap) nslab = cap;
    if (nslab < (a.n + (1 << 20) - 1) / (1 << 20)) nslab = (a.n + (1 << 20) - 1) / (1 << 20);
    a.slab_rows = (a.n + nslab - 1) / nslab;
    nslab = (a.n + a.slab_rows - 1) / a.slab_rows;
    if (nslab > 65535) return fail("epx_pooled_count_pass: %lld draws in one call, at most 65535 x 2^20", a.n);
    StreamSync sync{c->stream};
    if (upload_draws(c, src, &a.nm.draws)) return -1;
    const size_t n_hist = L * nt * 256;
    HIPCHK(c->count_ws.grow(n_hist + L + L * nt));
    a.hist = c->count_ws; a.n_nan = a.hist + n_hist;
    unsigned long long *prefix_d = a.n_nan + L;
    HIPCHK(hipMemsetAsync(a.hist, 0, (n_hist + L) * 8, c->stream));
    if (shift < 56) HIPCHK(hipMemcpyAsync(prefix_d, prefix, L * nt * 8, hipMemcpyHostToDevice, c->stream));
    a.prefix = prefix_d;
    if (launch(k_pooled_count, dim3((unsigned)ntile, (unsigned)nslab), dim3(EPX_QT_THREADS), lds, c->stream, a)) return -1;
    static_assert(sizeof(long long) == sizeof(unsigned long long), "counts are copied as they are");
    HIPCHK(hipMemcpyAsync(hist, a.hist, n_hist * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(n_nan, a.n_nan, L * 8, hipMemcpyDeviceToHost, c->stream));
    *n = a.n;
    return sync.finish();
}

int epx_predict(epx_ctx *c, int k0, int count, const int64_t *row_lim, const int32_t *row_group, const double *Xn,
                const double *yn, const double *theta, int S, double *out, int *nsamp) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    if (!row_lim) return fail("epx_predict: row_lim is required");
    if (check_walk_columns(c, "epx_predict")) return -1;
    int64_t n;
    if (new_row_count("epx_predict", k0, count, row_lim, &n)) return -1;
    const size_t D = c->D;
    DrawSource src;
    if (draw_source(c, "epx_predict", k0, count, theta, S, nullptr, &src)) return -1;
    if (nsamp) *nsamp = src.S;
    if (n == 0) return 0;
    if (!Xn || !out) return fail("epx_predict: Xn and out are required");
    if (yn)
        if (const int64_t i = bad_response(c, yn, n, false); i >= 0)
            return fail("epx_predict: row %lld: y = %g, the Bernoulli models take 0 or 1", (long long)i, yn[i]);
    // rows sorted by (site, group), stable: perm[sorted position] = row; then workgroups of <= 64 rows of one (site, group)
    std::vector<int> perm((size_t)n);
    std::vector<PredictWg> wg;
    if (cut_new_rows(c, "epx_predict", k0, count, row_lim, row_group, EPX_PR_WG_ROWS, perm.data(), wg)) return -1;
    PredictArgs a = bind_walk(c, k0, src.S);
    const size_t nn = (size_t)n, nwg = wg.size();
    HIPCHK(c->pred_ws.grow(nn * D + nn + nn * EPX_PR_COUNT));
    HIPCHK(c->pred_iws.grow(4 * nwg + nn));
    double *X_d = c->pred_ws, *y_d = X_d + nn * D, *out_d = y_d + nn;
    int *wg_d = c->pred_iws, *perm_d = wg_d + 4 * nwg;
    StreamSync sync{c->stream};          // (`perm` and `wg` are this frame's: the guard is declared behind them)
    if (upload_draws(c, src, &a.draws)) return -1;
    if (queue_new_rows(c, nn, Xn, yn, perm.data(), X_d, y_d, perm_d)) return -1;
    if (upload_items(c, wg, wg_d, &a.wg)) return -1;
    a.perm = perm_d; a.X = X_d; a.y = yn ? y_d : nullptr; a.out = out_d;
    if (launch(k_predict, dim3((unsigned)nwg), dim3(256), 0, c->stream, a)) return -1;
    HIPCHK(hipMemcpyAsync(out, out_d, nn * EPX_PR_COUNT * 8, hipMemcpyDeviceToHost, c->stream));
    return sync.finish();
}

int epx_predict_order_stats(epx_ctx *c, int k0, int count, const int64_t *row_lim, const int32_t *row_group, const double *Xn,
                            const int64_t *row_id, int what, uint64_t seed, const int64_t *ranks, int n_ranks,
                            const double *theta, int S, double *out, int *nsamp) {
    CTX(c);
    const char *who = "epx_predict_order_stats";
    if (check_range(c, k0, count)) return -1;
    if (check_walk_columns(c, who)) return -1;
    int64_t n;
    if (new_row_count(who, k0, count, row_lim, &n)) return -1;
    if (what != EPX_PO_F && what != EPX_PO_YREP)
        return fail("%s: what = %d, one of EPX_PO_F = %d, EPX_PO_YREP = %d", who, what, (int)EPX_PO_F, (int)EPX_PO_YREP);
    if (what == EPX_PO_YREP && !c->gauss)
        return fail("%s: EPX_PO_YREP is defined for the Gaussian family only: a Bernoulli-logit model's 0/1 replicate has no "
                    "useful quantile", who);
    if (check_rank_count(who, ranks, n_ranks)) return -1;
    if (n > 0 && (!Xn || !out)) return fail("%s: Xn and out are required", who);
    const size_t nn = (size_t)n, D = c->D;
    std::vector<uint32_t> ids;
    if (row_id) {
        ids.resize(nn);
        for (size_t i = 0; i < nn; ++i) {
            if (row_id[i] < 0 || row_id[i] >= (1ll << 32))
                return fail("%s: row %lld: row_id = %lld outside [0,2^32)", who, (long long)i, (long long)row_id[i]);
            ids[i] = (uint32_t)row_id[i];
        }
    }
    if (what != EPX_PO_YREP) ids.clear();                 // (checked all the same; only the replicates read them)
    PredOrderArgs a;
    DrawSource src;
    if (draw_source(c, who, k0, count, theta, S, nullptr, &src)) return -1;
    S = src.S;
    if (fill_ranks(who, ranks, n_ranks, S, a.rank)) return -1;
    a.p = bind_walk(c, k0, S);
    // the keys' share of the LDS: R rows of N(S) keys behind the walk's fixed part
    std::string lowered;                                  // what a refusal says of the variable, where it lowered the budget
    const size_t budget = lds_budget("EPX_PO_LDS_BYTES", pred_order_budget(a.p.m.KP), &lowered);
    size_t nmax = 0;                                      // the largest power of two of keys that fits: the largest S
    for (size_t m = 1; m * 8 <= budget; m *= 2) nmax = m;
    const auto too_many = [&](size_t most) {
        return fail("%s: S = %d draws per site, at most %d (a row's keys, padded to a power of two, are sorted in LDS%s)", who, S,
                    (int)most, lowered.c_str());
    };
    if ((size_t)S > nmax) return too_many(nmax);
    a.npad = pow2_pad(S, &a.lg);
    int R = 16;
    while (R > 1 && (size_t)R * a.npad * 8 > budget) R /= 2;
    if ((size_t)R * a.npad * 8 > budget) return too_many(0);      // (S = 1 under a budget below two keys)
    // rows sorted by (site, group), stable: perm[sorted position] = row; then work items of <= R rows of one (site, group)
    std::vector<int> perm(nn);
    std::vector<PredictWg> wg;
    if (cut_new_rows(c, who, k0, count, row_lim, row_group, R, perm.data(), wg)) return -1;
    if (wg.size() > 0x7fffffff) return fail("%s: %lld work items in one call, at most 2^31 - 1", who, (long long)wg.size());
    if (nsamp) *nsamp = S;                                // (behind the last refusal: a refusal writes nothing)
    if (n == 0) return 0;
    a.what = what; a.seed = seed; a.n_ranks = n_ranks;
    const size_t nwg = wg.size(), lds = pred_order_fixed_bytes(a.p.m.KP) + (size_t)R * a.npad * 8;
    a.nwg = (int)nwg;
    HIPCHK(c->pred_ws.grow(nn * D + nn * n_ranks));
    HIPCHK(c->pred_iws.grow(4 * nwg + nn + (ids.empty() ? 0 : nn)));
    double *X_d = c->pred_ws, *out_d = X_d + nn * D;
    int *wg_d = c->pred_iws, *perm_d = wg_d + 4 * nwg, *id_d = perm_d + nn;
    static_assert(sizeof(uint32_t) == sizeof(int), "the rows' stream indices lie in the int workspace");
    StreamSync sync{c->stream};          // (`ids`, `perm` and `wg` are this frame's: the guard is declared behind them)
    if (upload_draws(c, src, &a.p.draws)) return -1;
    if (queue_new_rows(c, nn, Xn, nullptr, perm.data(), X_d, nullptr, perm_d)) return -1;
    if (upload_items(c, wg, wg_d, &a.p.wg)) return -1;
    if (!ids.empty()) HIPCHK(hipMemcpyAsync(id_d, ids.data(), nn * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    a.p.perm = perm_d; a.p.X = X_d;
    a.row_id = ids.empty() ? nullptr : reinterpret_cast<const uint32_t *>(id_d);
    a.out = out_d;
    // (the kernel's registers leave room for two workgroups per compute unit, the LDS for one where the keys fill it)
    if (launch(k_predict_order, dim3(walk_grid(c, nwg, 2 * lds <= LDS_CAP ? 2 : 1)), dim3(256), lds, c->stream, a)) return -1;
    HIPCHK(hipMemcpyAsync(out, out_d, nn * n_ranks * 8, hipMemcpyDeviceToHost, c->stream));
    return sync.finish();
}

int epx_predict_new_group(epx_ctx *c, int k0, int count, uint64_t seed, long long t0, int R, long long n, const double *Xn,
                          const double *yn, const int32_t *row_group, int G, const int32_t *group_label,
                          const double *theta, int S, double *out, double *out_group, long long *N) {
    CTX(c);
    const char *who = "epx_predict_new_group";
    if (check_range(c, k0, count)) return -1;
    if (R < 1 || R > EPX_NGP_RMAX) return fail("%s: R must be in 1..%d (got %d)", who, (int)EPX_NGP_RMAX, R);
    if (check_walk_columns(c, who)) return -1;
    if (n < 0 || n > 0x7fffffff) return fail("%s: %lld rows in one call, between 0 and 2^31 - 1", who, n);
    if (G < 0 || (G > 0 && !group_label)) return fail("%s: G = %d groups need their labels", who, G);
    if (t0 < 0 || t0 > (1ll << 32)) return fail("%s: t0 = %lld outside [0,2^32]", who, t0);
    if (n > 0 && (!Xn || !out)) return fail("%s: Xn and out are required", who);
    for (int g = 0; g < G; ++g)
        if (group_label[g] < 0) return fail("%s: group %d: label %d is negative", who, g, (int)group_label[g]);
    // rows sorted by group, stable: perm[sorted position] = row
    std::vector<int> gfirst, perm((size_t)n), live;
    if (const int64_t i = sort_rows_by_group(0, n, row_group, G, perm.data(), gfirst); i >= 0)
        return fail("%s: row %lld: group %d outside [0,%d)", who, (long long)i, row_group ? (int)row_group[i] : 0, G);
    if (yn)
        if (const int64_t i = bad_response(c, yn, n, true); i >= 0)
            return fail("%s: row %lld: y = %g, %s", who, (long long)i, yn[i],
                        c->gauss ? "the Gaussian models take finite responses" : "the Bernoulli models take 0 or 1");
    for (int g = 0; g < G; ++g)
        if (gfirst[(size_t)g + 1] > gfirst[g]) live.push_back(g);
    NewGroupArgs a;
    DrawSource src;
    if (draw_source(c, who, k0, count, theta, S, nullptr, &src)) return -1;
    const long long T = (long long)count * src.S;
    if (t0 + T > (1ll << 32))
        return fail("%s: pooled draws [%lld,%lld) outside [0,2^32)", who, t0, t0 + T);
    a.N = T * R;
    if (N) *N = a.N;
    if (n == 0) return 0;
    a.m = predict_model(c);
    a.E = c->model == EPX_M1B_SG ? 1 : 1 + c->D; a.lap = c->model == EPX_M5B_SG;
    a.R = R; a.t0 = t0; a.seed = seed; a.n = (int)n; a.G = G;
    a.chunk_slabs = newgroup_chunk_slabs(a.N);
    const long long chunk = (long long)a.chunk_slabs * 16;
    a.nchunk = (a.N + chunk - 1) / chunk;
    a.nitem = (long long)live.size() * a.nchunk;
    const size_t nn = (size_t)n, D = c->D, nG = (size_t)G, nch = (size_t)a.nchunk;
    HIPCHK(c->pred_ws.grow(nn * D + nn + nch * nn * EPX_PR_COUNT + nch * nG + nn * EPX_PR_COUNT + nG * EPX_NG_COUNT));
    HIPCHK(c->pred_iws.grow(nn + (nG + 1) + nG + live.size()));
    double *X_d = c->pred_ws, *y_d = X_d + nn * D, *rows_d = y_d + nn, *grp_d = rows_d + nch * nn * EPX_PR_COUNT;
    double *out_d = grp_d + nch * nG, *outg_d = out_d + nn * EPX_PR_COUNT;
    int *perm_d = c->pred_iws, *gfirst_d = perm_d + nn, *label_d = gfirst_d + nG + 1, *live_d = label_d + nG;
    StreamSync sync{c->stream};          // (`perm`, `gfirst` and `live` are this frame's: the guard is declared behind them)
    if (upload_draws(c, src, &a.draws)) return -1;
    if (queue_new_rows(c, nn, Xn, yn, perm.data(), X_d, y_d, perm_d)) return -1;
    HIPCHK(hipMemcpyAsync(gfirst_d, gfirst.data(), (nG + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(label_d, group_label, nG * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(live_d, live.data(), live.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    a.perm = perm_d; a.gfirst = gfirst_d; a.label = label_d; a.live = live_d;
    a.X = X_d; a.y = yn ? y_d : nullptr;
    a.part_rows = rows_d; a.part_grp = grp_d; a.out = out_d; a.out_group = outg_d;
    if (launch(k_newgroup, dim3(walk_grid(c, (size_t)a.nitem, 4)), dim3(256), 0, c->stream, a)) return -1;
    const long long mblocks = ((long long)n + G + 255) / 256;
    if (launch(k_newgroup_merge, dim3((unsigned)(mblocks < 65536 ? mblocks : 65536)), dim3(256), 0, c->stream, a)) return -1;
    HIPCHK(hipMemcpyAsync(out, out_d, nn * EPX_PR_COUNT * 8, hipMemcpyDeviceToHost, c->stream));
    if (out_group) HIPCHK(hipMemcpyAsync(out_group, outg_d, nG * EPX_NG_COUNT * 8, hipMemcpyDeviceToHost, c->stream));
    return sync.finish();
}

// LDS of the per-row PSIS stage (psis.h): 16 rows' scratch
static size_t psis_lds_bytes(int M) { return (size_t)16 * psis_scratch_doubles(M) * 8; }

int epx_loo(epx_ctx *c, int k0, int count, const double *theta, int S, double *out, int *nsamp) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    if (check_walk_columns(c, "epx_loo")) return -1;
    if (!out) return fail("epx_loo: out is required");
    LooArgs a;
    DrawSource src;
    if (draw_source(c, "epx_loo", k0, count, theta, S, nullptr, &src)) return -1;
    S = src.S;
    a.p = bind_walk(c, k0, S);
    a.p.X = c->X; a.y8 = c->y; a.yd = c->yd;
    a.M = psis_tail_length(S); a.mfit = psis_fit_points(a.M);
    a.stride = loo_stride(S);
    // LDS: [coefficient slab | log sigma, sigma of the slab | PSIS scratch | tiles]; the tiles go to the workspace when
    // not even one fits
    const size_t cap = lds_budget("EPX_LOO_LDS_BYTES", LDS_CAP - 1024);
    const size_t fixed = ((size_t)a.p.m.KP * 16 + 32) * 8 + psis_lds_bytes(a.M), tile = (size_t)16 * a.stride * 8;
    if (a.mfit > PSIS_FIT_MAX || fixed > LDS_CAP - 1024)
        return fail("epx_loo: S = %d draws: the tail of %d draws per row does not fit the LDS", S, a.M);
    a.tiles = fixed + 4 * tile <= cap ? 4 : fixed + 2 * tile <= cap ? 2 : fixed + tile <= cap ? 1 : 0;
    const bool in_lds = a.tiles > 0;
    if (!in_lds) a.tiles = 1;
    const size_t lds = fixed + (in_lds ? a.tiles * tile : 0);
    // work items: up to 16 x tiles rows of one (site, group), in the context's row order
    const int item = 16 * a.tiles;
    if (check_ctx_rows(c, "epx_loo")) return -1;
    if (nsamp) *nsamp = S;                                // (behind the last refusal: a refusal writes nothing)
    std::vector<PredictWg> wg;
    cut_ctx_rows(c, k0, count, item, wg);
    a.row0 = c->k_lim[k0];
    const size_t rows = (size_t)(c->k_lim[k0 + count] - c->k_lim[k0]), nwg = wg.size();
    const unsigned grid = walk_grid(c, nwg, in_lds ? 4 : 2);       // (the LDS holds one or two workgroups per compute unit)
    const size_t n_out = rows * EPX_LO_COUNT, n_slab = in_lds ? 0 : (size_t)grid * item * a.stride;
    HIPCHK(c->loo_ws.grow(n_out + n_slab));
    HIPCHK(c->pred_iws.grow(4 * nwg));
    a.out = c->loo_ws; a.slab = in_lds ? nullptr : c->loo_ws + n_out;
    a.nwg = (int)nwg;
    StreamSync sync{c->stream};          // (`wg` is this frame's: the guard is declared behind it)
    if (upload_draws(c, src, &a.p.draws)) return -1;
    if (upload_items(c, wg, c->pred_iws, &a.p.wg)) return -1;
    if (launch(k_loo, dim3(grid), dim3(256), lds, c->stream, a)) return -1;
    HIPCHK(hipMemcpyAsync(out, a.out, n_out * 8, hipMemcpyDeviceToHost, c->stream));
    return sync.finish();
}

int epx_ppc(epx_ctx *c, int k0, int count, uint64_t seed, long long row0, const double *theta, int S, double *out_groups,
            double *out_sites, double *out_draws, int *nsamp) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    if (check_walk_columns(c, "epx_ppc")) return -1;
    if (!out_groups) return fail("epx_ppc: out_groups is required");
    if (check_ctx_rows(c, "epx_ppc")) return -1;
    if (row0 < 0 || row0 + (long long)c->k_lim[k0 + count] >= (1ll << 32))
        return fail("epx_ppc: row0 = %lld puts the rows of the call at [%lld,%lld), outside [0,2^32 - 1)", row0,
                    row0 + (long long)c->k_lim[k0], row0 + (long long)c->k_lim[k0 + count]);
    PpcArgs a;
    DrawSource src;
    if (draw_source(c, "epx_ppc", k0, count, theta, S, nullptr, &src)) return -1;
    S = src.S;
    a.p = bind_walk(c, k0, S);
    if (S > ppc_max_draws(a.p.m.KP))
        return fail("epx_ppc: S = %d draws, at most %d (a group's 3 x S per-draw sums are kept in LDS)", S,
                    ppc_max_draws(a.p.m.KP));
    if (nsamp) *nsamp = S;                                // (behind the last refusal: a refusal writes nothing)
    a.p.X = c->X; a.y8 = c->y; a.yd = c->yd;
    a.seed = seed; a.row0 = row0; a.count = count;
    // work items: the groups of the range, whole, in the context's order; site_first: the first of every site
    std::vector<PredictWg> wg;
    std::vector<int> site_first;
    cut_ctx_rows(c, k0, count, 0, wg, &site_first);
    const size_t ng_all = wg.size(), n_draws = ng_all * 3 * (size_t)S, n_grp = ng_all * EPX_PC_COUNT,
                 n_site = (size_t)count * EPX_PC_COUNT, lds = ppc_lds_bytes(a.p.m.KP, S);
    a.ngroups = (int)ng_all;
    HIPCHK(c->ppc_ws.grow(n_draws + n_grp + n_site));
    HIPCHK(c->pred_iws.grow(4 * ng_all + site_first.size()));
    a.per_draw = c->ppc_ws; a.out_groups = a.per_draw + n_draws; a.out_sites = a.out_groups + n_grp;
    int *wg_d = c->pred_iws, *first_d = wg_d + 4 * ng_all;
    StreamSync sync{c->stream};          // (`wg` and `site_first` are this frame's: the guard is declared behind them)
    if (upload_draws(c, src, &a.p.draws)) return -1;
    if (upload_items(c, wg, wg_d, &a.p.wg)) return -1;
    HIPCHK(hipMemcpyAsync(first_d, site_first.data(), site_first.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    a.site_first = first_d;
    if (launch(k_ppc, dim3(walk_grid(c, ng_all, 4)), dim3(256), lds, c->stream, a)) return -1;
    if (launch(k_ppc_sites, dim3((unsigned)((count + 15) / 16)), dim3(256), 0, c->stream, a)) return -1;
    HIPCHK(hipMemcpyAsync(out_groups, a.out_groups, n_grp * 8, hipMemcpyDeviceToHost, c->stream));
    if (out_sites) HIPCHK(hipMemcpyAsync(out_sites, a.out_sites, n_site * 8, hipMemcpyDeviceToHost, c->stream));
    if (out_draws) HIPCHK(hipMemcpyAsync(out_draws, a.per_draw, n_draws * 8, hipMemcpyDeviceToHost, c->stream));
    return sync.finish();
}

int epx_site_evidence(epx_ctx *c, int k0, int count, uint64_t seed, long long site0, const double *theta, int S, int chains,
                      double *out, double *out_terms, double *elapsed_ms) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    if (check_walk_columns(c, "epx_site_evidence")) return -1;
    if (!out) return fail("epx_site_evidence: out is required");
    if (check_ctx_rows(c, "epx_site_evidence")) return -1;
    if (site0 < 0 || site0 + (long long)c->K >= (1ll << 31))
        return fail("epx_site_evidence: site0 = %lld puts the context's %d sites outside [0,2^31)", site0, c->K);
    EvidenceArgs a;
    a.m = predict_model(c);
    const int P = c->P;
    if (P > evidence_max_coords(a.m.KP))
        return fail("epx_site_evidence: P = %d sampled coordinates, at most %d at D = %d (the packed factor of the proposal "
                    "and the slab's workspace are kept in LDS)", P, evidence_max_coords(a.m.KP), c->D);
    DrawSource src;
    const int chains_given = chains;
    if (draw_source(c, "epx_site_evidence", k0, count, theta, S, &chains, &src)) return -1;
    if (!theta && chains_given != 0 && chains_given != src.chains)       // (the caller sized out_terms by its chains)
        return fail("epx_site_evidence: chains = %d given, the last sampling call left draws of %d chains", chains_given,
                    src.chains);
    S = src.S; chains = src.chains;
    a.S = S; a.chains = chains; a.n = S / chains; a.nh = a.n / 2;
    const long long nF = (long long)a.nh * chains;
    a.N1 = S - (int)nF;
    if (nF < 2ll * P)
        return fail("epx_site_evidence: the fit set holds %lld draws (the first %d of each of %d chains), the proposal of "
                    "P = %d coordinates needs at least %d", nF, a.nh, chains, P, 2 * P);
    a.M = psis_tail_length(a.N1); a.mfit = psis_fit_points(a.M);
    const size_t lds_bridge = evidence_bridge_doubles(a.N1, psis_scratch_doubles(a.M)) * 8;
    if (a.mfit > PSIS_FIT_MAX || lds_bridge > LDS_CAP - 1024)
        return fail("epx_site_evidence: N1 = %d estimation draws: the terms of the bridge (%zu bytes) do not fit the LDS",
                    a.N1, lds_bridge);
    a.k0 = k0; a.pg = c->model == EPX_M1B_SG ? 1 : 1 + c->D;
    a.site_g0 = site_g0(c);
    a.X = c->X; a.y8 = c->y; a.yd = c->yd;
    a.cav_Om = c->cav_Om; a.cav_mu = c->cav_mu;
    a.seed = seed; a.site0 = site0;
    // the groups of the range, whole, in the context's order; site_first: the first of every site
    std::vector<PredictWg> wg;
    std::vector<int> site_first;
    cut_ctx_rows(c, k0, count, 0, wg, &site_first);
    const size_t ng_all = wg.size(), fitw = evidence_fit_doubles(P), n_fit = (size_t)count * fitw,
                 n_terms = (size_t)count * 2 * a.N1, n_out = (size_t)count * EPX_EV_COUNT,
                 n_prop = out_terms ? (size_t)count * a.N1 * P : 0;
    HIPCHK(c->ev_ws.grow(n_fit + n_terms + n_out + n_prop));
    HIPCHK(c->pred_iws.grow(4 * ng_all + site_first.size()));
    a.fit = c->ev_ws; a.terms = a.fit + n_fit; a.out = a.terms + n_terms; a.prop = out_terms ? a.out + n_out : nullptr;
    int *wg_d = c->pred_iws, *first_d = wg_d + 4 * ng_all;
    const size_t lds_fit = (evidence_packed(P) + 2 * P + 2) * 8, lds_terms = evidence_terms_doubles(P, a.m.KP) * 8;
    StreamSync sync{c->stream};          // (`wg` and `site_first` are this frame's: the guard is declared behind them)
    if (upload_draws(c, src, &a.draws)) return -1;
    if (upload_items(c, wg, wg_d, &a.wg)) return -1;
    HIPCHK(hipMemcpyAsync(first_d, site_first.data(), site_first.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    a.site_first = first_d;
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    const dim3 sites((unsigned)count), threads(256);
    if (launch(k_ev_fit, sites, threads, lds_fit, c->stream, a) || launch(k_ev_terms, sites, threads, lds_terms, c->stream, a) ||
        launch(k_ev_bridge, sites, threads, lds_bridge, c->stream, a))
        return -1;
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipMemcpyAsync(out, a.out, n_out * 8, hipMemcpyDeviceToHost, c->stream));
    if (out_terms) {
        // per site [l1, l2 | m, L packed | proposal draws]: three strided copies
        const size_t w_t = (size_t)2 * a.N1, w_f = fitw - 2, w_p = (size_t)a.N1 * P, width = (w_t + w_f + w_p) * 8;
        HIPCHK(hipMemcpy2DAsync(out_terms, width, a.terms, w_t * 8, w_t * 8, (size_t)count, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpy2DAsync(out_terms + w_t, width, a.fit, fitw * 8, w_f * 8, (size_t)count, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpy2DAsync(out_terms + w_t + w_f, width, a.prop, w_p * 8, w_p * 8, (size_t)count, hipMemcpyDeviceToHost,
                                c->stream));
    }
    if (sync.finish()) return -1;
    if (elapsed_ms) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        *elapsed_ms = ms;
    }
    return 0;
}

int epx_draw_diagnostics(epx_ctx *c, int k0, int count, const double *theta, int S, int chains, double *out, int *nsamp) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    if (!out) return fail("epx_draw_diagnostics: out is required");
    const size_t P = c->P;
    DiagArgs a;
    DrawSource src;
    if (draw_source(c, "epx_draw_diagnostics", k0, count, theta, S, &chains, &src)) return -1;
    S = src.S; chains = src.chains;
    a.k0 = k0; a.chains = chains; a.nkeep = S / chains; a.P = c->P;
    a.d = c->d; a.pg = c->pg; a.site_g0 = site_g0(c);
    const int n = 2 * chains * (a.nkeep / 2);
    a.tau_min = n > 1 ? 1.0 / log10((double)n) : 0.0;
    a.in_lds = diag_lds_doubles(chains, a.nkeep, true) * 8 + 1024 <= LDS_CAP;
    const size_t lds = diag_lds_doubles(chains, a.nkeep, a.in_lds != 0) * 8;
    StreamSync sync{c->stream};
    if (upload_draws(c, src, &a.draws)) return -1;
    const size_t nout = (size_t)count * P * EPX_DG_COUNT;
    HIPCHK(c->diag_out.grow(nout));
    a.out = c->diag_out;
    const dim3 grid((unsigned)count, (unsigned)((P + EPX_DG_TILE - 1) / EPX_DG_TILE));
    if (launch(k_draw_diag, grid, dim3(256), lds, c->stream, a)) return -1;
    HIPCHK(hipMemcpyAsync(out, a.out, nout * 8, hipMemcpyDeviceToHost, c->stream));
    if (nsamp) *nsamp = n;
    return sync.finish();
}

int epx_draw_rank_diagnostics(epx_ctx *c, int k0, int count, const double *theta, int S, int chains, double *out,
                              int *nsamp) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    if (!out) return fail("epx_draw_rank_diagnostics: out is required");
    const size_t P = c->P;
    RankDiagArgs a;
    DrawSource src;
    if (draw_source(c, "epx_draw_rank_diagnostics", k0, count, theta, S, &chains, &src)) return -1;
    S = src.S; chains = src.chains;
    if (chains > EPX_DG_MAX_CHAINS)
        return fail("epx_draw_rank_diagnostics: %d chains, at most %d", chains, (int)EPX_DG_MAX_CHAINS);
    a.k0 = k0; a.chains = chains; a.nkeep = S / chains; a.P = c->P;
    a.d = c->d; a.pg = c->pg; a.site_g0 = site_g0(c);
    const long long n = 2ll * chains * (a.nkeep / 2);
    if (n > EPX_RD_MAX_DRAWS)
        return fail("epx_draw_rank_diagnostics: %lld used draws per site, at most %d (a coordinate's keys, draw indices and "
                    "scores are kept in LDS)", n, (int)EPX_RD_MAX_DRAWS);
    if ((size_t)count * P > 0x7fffffffull)
        return fail("epx_draw_rank_diagnostics: %d sites x %zu coordinates in one call, at most 2^31 - 1", count, P);
    a.tau_min = n > 1 ? 1.0 / log10((double)n) : 0.0;
    const size_t lds = rank_lds_bytes((int)n);
    StreamSync sync{c->stream};
    if (upload_draws(c, src, &a.draws)) return -1;
    const size_t nout = (size_t)count * P * EPX_RD_COUNT;
    HIPCHK(c->rank_out.grow(nout));
    a.out = c->rank_out;
    if (launch(k_rank_diag, dim3((unsigned)((size_t)count * P)), dim3(EPX_RD_THREADS), lds, c->stream, a)) return -1;
    HIPCHK(hipMemcpyAsync(out, a.out, nout * 8, hipMemcpyDeviceToHost, c->stream));
    if (nsamp) *nsamp = (int)n;
    return sync.finish();
}

int epx_pooled_moments(epx_ctx *c, int k0, int count, const double *center, const double *theta, int S, int want_scatter,
                       double *sum, double *scatter, long long *n) {
    CTX(c);
    if (check_range(c, k0, count)) return -1;
    if (!sum || !n) return fail("epx_pooled_moments: sum and n are required");
    if (want_scatter && !scatter) return fail("epx_pooled_moments: want_scatter without a scatter array");
    const size_t d = c->d;
    PooledArgs a;
    DrawSource src;
    if (draw_source(c, "epx_pooled_moments", k0, count, theta, S, nullptr, &src)) return -1;
    StreamSync sync{c->stream};
    if (upload_draws(c, src, &a.draws)) return -1;
    a.d = c->d; a.P = c->P; a.nt = (c->d + 15) / 16; a.want_scatter = want_scatter ? 1 : 0;
    a.n = (long long)count * src.S;
    // the slabs depend on (n, d) alone: the same partition, hence the same bits, on every call.  About 2048 workgroups
    // (eight per compute unit) of at least 128 records each; whole groups of 16 records (four per wave and step)
    const int pairs = want_scatter ? a.nt * (a.nt + 1) / 2 : a.nt;
    const long long max_slabs = 2048 / pairs > 1 ? 2048 / pairs : 1;
    a.slab_rows = (a.n + max_slabs - 1) / max_slabs;
    if (a.slab_rows < 128) a.slab_rows = 128;
    a.slab_rows = (a.slab_rows + 15) / 16 * 16;
    a.nslab = (int)((a.n + a.slab_rows - 1) / a.slab_rows);
    const size_t n_ps = want_scatter ? (size_t)a.nslab * pairs * 256 : 0, n_pm = (size_t)a.nslab * a.nt * 16;
    HIPCHK(c->pooled_ws.grow(n_ps + n_pm + d * d + 2 * d));
    a.part_scatter = c->pooled_ws; a.part_sum = a.part_scatter + n_ps;
    a.out_scatter = a.part_sum + n_pm; a.out_sum = a.out_scatter + d * d;
    double *center_d = a.out_sum + d;
    if (center) HIPCHK(hipMemcpyAsync(center_d, center, d * 8, hipMemcpyHostToDevice, c->stream));
    a.center = center ? center_d : nullptr;
    if (launch(k_pooled_partial, dim3(pairs, a.nslab), dim3(256), 0, c->stream, a)) return -1;
    const int nout = (int)((want_scatter ? d * d : 0) + d);
    if (launch(k_pooled_final, dim3((nout + 255) / 256), dim3(256), 0, c->stream, a)) return -1;
    HIPCHK(hipMemcpyAsync(sum, a.out_sum, d * 8, hipMemcpyDeviceToHost, c->stream));
    if (want_scatter) HIPCHK(hipMemcpyAsync(scatter, a.out_scatter, d * d * 8, hipMemcpyDeviceToHost, c->stream));
    *n = a.n;
    return sync.finish();
}

static int launch_global(epx_ctx *c, const double *packed_dev, double df, int want_moments,
                         const double *tgt = nullptr, double *crit = nullptr) {
    GlobalArgs a;
    a.tgt = tgt; a.crit = crit;
    a.want_moments = want_moments;
    a.packed = packed_dev; a.Q0 = c->Q0; a.r0 = c->r0; a.df = df;
    a.Q = c->Q; a.r = c->r; a.S = c->S; a.m = c->m; a.flag = c->iflags;
    // (one block, but the workspace is sized for the cavities that follow: it does not grow between the two)
    return launch_dense(k_global, 1, c->stream, c->dense_ws, c->d, c->K, a);
}

// Queued: one damping trial -- the global approximation from the packed sums at `df`, then every site's cavity against it.
// (epx_damped_trial queues the two halves itself: it looks at the global check in between.)
static int launch_trial(epx_ctx *c, const double *packed_dev, double df, int want_moments,
                        const double *tgt = nullptr, double *crit = nullptr) {
    if (launch_global(c, packed_dev, df, want_moments, tgt, crit)) return -1;
    return launch_proposal_cavities(c, df, 0, c->K);
}

// The packed sums a trial reads: the caller's host array, queued for copy into c->packed (behind the caller's
// StreamSync); else the caller's device array; else c->packed, the sums of the last epx_site_sums on this rank.
static int trial_sums(epx_ctx *c, const double *packed_host, const double *packed_dev, const double **pk) {
    *pk = packed_host || !packed_dev ? c->packed : packed_dev;
    if (packed_host) HIPCHK(hipMemcpyAsync(c->packed, packed_host, (size_t)2 * (c->d * c->d + c->d) * 8, hipMemcpyHostToDevice, c->stream));
    return 0;
}

int epx_damped_trial(epx_ctx *c, double df, const double *packed_host, const double *packed_dev,
                     int *global_pd, int *cav_pd, int *first_bad) {
    CTX(c);
    int h[4] = {0, 0, -1, 0};
    const double *pk;
    StreamSync global_sync{c->stream};
    if (trial_sums(c, packed_host, packed_dev, &pk)) return -1;
    c->last_df = df;
    if (launch_global(c, pk, df, 0)) return -1;
    HIPCHK(hipMemcpyAsync(h, c->iflags, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (global_sync.finish()) return -1;
    *global_pd = h[0];
    *cav_pd = 0;
    if (first_bad) *first_bad = -1;
    if (!h[0]) return 0;           // the documented early exit: cavities run only behind a positive definite global check
    StreamSync sync{c->stream};
    if (launch_proposal_cavities(c, df, 0, c->K)) return -1;
    hipLaunchKernelGGL(k_all_flags, dim3(1), dim3(256), 0, c->stream, c->flags, 0, c->K, c->iflags + 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h + 1, c->iflags + 1, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (sync.finish()) return -1;
    *cav_pd = h[1];
    if (first_bad) *first_bad = h[2];
    return 0;
}

int epx_update_trial(epx_ctx *c, double df, int reduce_sums, int site_base, double *stat_sum, int n_sum,
                     double *stat_max, int n_max, int want_moments, int *global_pd, int *cav_pd,
                     int64_t *first_bad, double *S, double *m) {
    CTX(c);
    const bool bound = c->comm || c->comm_ext;
    TrialStats st;
    if (trial_stats(n_sum, n_max, bound ? c->comm_size : 1, bound ? c->comm_rank : 0, &st)) return -1;
    const int len = 2 * (c->d * c->d + c->d);
    const size_t next = st.count();
    double *ext_d = c->packed + len, *trial_d = ext_d + TRIAL_FLAGS_AT;
    // (the host ends of the queued copies stand in front of the guard: they outlive its synchronisation on every exit)
    std::vector<double> ext(next + 1, 0.0);
    double tf[3] = {0, 0, 0};
    StreamSync sync{c->stream};
    if (reduce_sums) {
        st.pack(stat_sum, stat_max, ext.data());
        if (next) HIPCHK(hipMemcpyAsync(ext_d, ext.data(), next * 8, hipMemcpyHostToDevice, c->stream));
        if (queue_site_sums(c, k_site_sums_partial, len, c->Qi, c->ri, c->dQi, c->dri, c->packed)) return -1;
        // the ONE reduction of the iteration (method.py:1073-1074; affine in df, so it serves every trial)
        if (epx_comm_allreduce_dev(c, c->packed, len + next, EPX_OP_SUM)) return -1;
    }
    c->last_df = df;
    if (launch_trial(c, c->packed, df, want_moments)) return -1;
    hipLaunchKernelGGL(k_trial_flags, dim3(1), dim3(256), 0, c->stream, c->flags, c->K, site_base, c->iflags, trial_d);
    HIPCHK(hipGetLastError());
    if (epx_comm_allreduce_dev(c, trial_d, 3, EPX_OP_MIN)) return -1;
    HIPCHK(hipMemcpyAsync(tf, trial_d, sizeof tf, hipMemcpyDeviceToHost, c->stream));
    if (reduce_sums && next) HIPCHK(hipMemcpyAsync(ext.data(), ext_d, next * 8, hipMemcpyDeviceToHost, c->stream));
    if (want_moments && S) HIPCHK(hipMemcpyAsync(S, c->S, (size_t)c->d * c->d * 8, hipMemcpyDeviceToHost, c->stream));
    if (want_moments && m) HIPCHK(hipMemcpyAsync(m, c->m, (size_t)c->d * 8, hipMemcpyDeviceToHost, c->stream));
    if (sync.finish()) return -1;                   // the one synchronisation of the trial
    *global_pd = tf[0] != 0.0;
    *cav_pd = tf[1] != 0.0;
    if (first_bad) *first_bad = TrialStats::first_bad(tf[2]);
    if (reduce_sums) st.unpack(ext.data(), stat_sum, stat_max);
    return 0;
}

int epx_damp_sweep(epx_ctx *c, int ndf, const double *dfs, const double *packed_host, const double *packed_dev,
                   const double *m_target, const double *S_target, double half_logdet_S_target,
                   const double *samp_mean, const double *samp_scatter, int n_samp, double *out) {
    CTX(c);
    if (ndf < 1 || !dfs || !m_target || !S_target || !out) return fail("damp sweep: missing argument");
    const size_t d = c->d, d2 = d * d, ntgt = 2 * (d + d2) + 2;
    HIPCHK(c->sweep_buf.grow(ntgt + (size_t)ndf * 5));
    std::vector<double> h(ntgt, 0.0);
    memcpy(h.data(), m_target, d * 8);
    memcpy(h.data() + d, S_target, d2 * 8);
    const bool have_samp = samp_mean && samp_scatter && n_samp > 0;
    if (have_samp) { memcpy(h.data() + d + d2, samp_mean, d * 8); memcpy(h.data() + 2 * d + d2, samp_scatter, d2 * 8); }
    h[2 * (d + d2)] = half_logdet_S_target;
    h[2 * (d + d2) + 1] = have_samp ? (double)n_samp : 0.0;
    StreamSync sync{c->stream};
    HIPCHK(hipMemcpyAsync(c->sweep_buf, h.data(), ntgt * 8, hipMemcpyHostToDevice, c->stream));
    const double *pk;
    if (trial_sums(c, packed_host, packed_dev, &pk)) return -1;
    double *crit = c->sweep_buf + ntgt;
    // every trial back to back on the stream, one synchronisation at the end
    for (int i = 0; i < ndf; ++i) {
        if (launch_trial(c, pk, dfs[i], 1, c->sweep_buf, crit + (size_t)i * 5)) return -1;
        hipLaunchKernelGGL(k_all_flags, dim3(1), dim3(256), 0, c->stream, c->flags, 0, c->K, c->iflags + 1);
        hipLaunchKernelGGL(k_sweep_flag, dim3(1), dim3(64), 0, c->stream, c->iflags + 1, crit + (size_t)i * 5);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(out, crit, (size_t)ndf * 5 * 8, hipMemcpyDeviceToHost, c->stream));
    c->last_df = dfs[ndf - 1];       // (in front of the synchronisation: the good path ends with it; the orders differ only if it fails)
    return sync.finish();
}

int epx_accept(epx_ctx *c, double df) {
    CTX(c);
    // no synchronisation: every later use is ordered behind it on the context's stream (the
    // synchronous copies of the accessors run on the legacy default stream, which waits for it)
    return queue_site_axpy(c, c->Qi, c->ri, df);
}

int epx_global_moments(epx_ctx *c, double *S, double *m) {
    CTX(c);
    int ok = 0;
    StreamSync sync{c->stream};
    if (launch_global(c, nullptr, 0.0, 1)) return -1;
    HIPCHK(hipMemcpyAsync(&ok, c->iflags, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (sync.finish()) return -1;
    if (!ok) return fail("global precision is not positive definite");
    return copy_pair(c, c->S, c->m, 0, 1, S, m);
}

int epx_force_pd(epx_ctx *c, double df, double thresh, double min_eig_target, uint8_t *forced) {
    CTX(c);
    ForceArgs a;
    a.Qi = c->Qi; a.dQi = c->dQi; a.df = df; a.thresh = thresh; a.target = min_eig_target;
    a.forced = c->flags; a.min_eig = c->min_eig;
    if (launch_dense(k_force_pd, c->K, c->stream, c->dense_ws, c->d, c->K, a)) return -1;
    return fetch_flags(c, 0, c->K, forced);
}

// ------------------------------------------------------ stand-alone util ops
static int need_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail("no HIP device available: libepx has no CPU fallback");
    if (device < 0 || device >= ndev) return fail("device %d out of range", device);
    HIPCHK(hipSetDevice(device));
    return 0;
}

// the stand-alone entry points run on the device they are given and leave the calling thread's
// current device as they found it (a rank of a multi-GPU job keeps its own GPU current)
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

int epx_invert_normal_params(int device, int d, int nb, double *A, double *b, int cho_form, int32_t *info) {
    DeviceGuard guard;
    if (need_device(device)) return -1;
    if (d < 1 || nb < 1) return fail("bad sizes");
    InvertArgs a;
    a.cho_form = cho_form;
    DevBuf<double> ws, Ad, bd;
    DevBuf<int32_t> infod;
    HIPCHK(Ad.alloc((size_t)nb * d * d));
    HIPCHK(infod.alloc(nb));
    HIPCHK(hipMemcpy(Ad, A, (size_t)nb * d * d * 8, hipMemcpyHostToDevice));
    if (b) { HIPCHK(bd.alloc((size_t)nb * d)); HIPCHK(hipMemcpy(bd, b, (size_t)nb * d * 8, hipMemcpyHostToDevice)); }
    a.A = Ad; a.b = bd; a.info = infod;
    if (launch_dense(k_invert, nb, 0, ws, d, nb, a)) return -1;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(A, Ad, (size_t)nb * d * d * 8, hipMemcpyDeviceToHost));
    if (b) HIPCHK(hipMemcpy(b, bd, (size_t)nb * d * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(info, infod, nb * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

int epx_olse(int device, int d, int nb, double *S, int n, const double *P, int32_t *info) {
    DeviceGuard guard;
    if (need_device(device)) return -1;
    if (d < 1 || nb < 1) return fail("bad sizes");
    OlseArgs a;
    a.n = n;
    DevBuf<double> ws, Sd, Pd;
    DevBuf<int32_t> infod;
    HIPCHK(Sd.alloc((size_t)nb * d * d));
    HIPCHK(infod.alloc(nb));
    HIPCHK(hipMemcpy(Sd, S, (size_t)nb * d * d * 8, hipMemcpyHostToDevice));
    if (P) { HIPCHK(Pd.alloc((size_t)nb * d * d)); HIPCHK(hipMemcpy(Pd, P, (size_t)nb * d * d * 8, hipMemcpyHostToDevice)); }
    a.S = Sd; a.P = Pd; a.info = infod;
    if (launch_dense(k_olse, nb, 0, ws, d, nb, a)) return -1;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(S, Sd, (size_t)nb * d * d * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(info, infod, nb * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

int epx_psis_rows(int device, long long n, int S, const double *ll, double *out) {
    DeviceGuard guard;
    if (need_device(device)) return -1;
    if (n < 0 || S < 1) return fail("epx_psis_rows: n = %lld rows of S = %d draws", n, S);
    if (n == 0) return 0;
    if (!ll || !out) return fail("epx_psis_rows: ll and out are required");
    PsisRowsArgs a;
    a.n = n; a.S = S; a.M = psis_tail_length(S); a.mfit = psis_fit_points(a.M);
    const size_t lds = psis_lds_bytes(a.M);
    if (a.mfit > PSIS_FIT_MAX || lds > LDS_CAP - 1024)
        return fail("epx_psis_rows: S = %d draws: the tail of %d draws per row does not fit the LDS", S, a.M);
    DevBuf<double> lld, outd;
    HIPCHK(lld.alloc((size_t)n * S));
    HIPCHK(outd.alloc((size_t)n * 3));
    HIPCHK(hipMemcpy(lld, ll, (size_t)n * S * 8, hipMemcpyHostToDevice));
    a.ll = lld; a.out = outd;
    const long long steps = (n + 15) / 16;
    if (launch(k_psis_rows, dim3((unsigned)(steps < 65536 ? steps : 65536)), dim3(256), lds, 0, a)) return -1;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, outd, (size_t)n * 3 * 8, hipMemcpyDeviceToHost));
    return 0;
}

int epx_rank_normalize(int device, long long m, int n, const double *x, int fold, double *rank_out, double *z_out) {
    DeviceGuard guard;
    if (need_device(device)) return -1;
    if (m < 0 || m > 0x7fffffffll || n < 1) return fail("epx_rank_normalize: m = %lld series of n = %d values", m, n);
    if (n > EPX_RD_MAX_DRAWS)
        return fail("epx_rank_normalize: n = %d values per series, at most %d (a series' keys, indices and scores are kept "
                    "in LDS)", n, (int)EPX_RD_MAX_DRAWS);
    if (m == 0) return 0;
    if (!x || !rank_out || !z_out) return fail("epx_rank_normalize: x, rank_out and z_out are required");
    RankNormArgs a;
    a.n = n; a.fold = fold ? 1 : 0;
    const size_t total = (size_t)m * n, lds = rank_lds_bytes(n);
    DevBuf<double> xd, rd, zd;
    HIPCHK(xd.alloc(total));
    HIPCHK(rd.alloc(total));
    HIPCHK(zd.alloc(total));
    HIPCHK(hipMemcpy(xd, x, total * 8, hipMemcpyHostToDevice));
    a.x = xd; a.rank = rd; a.z = zd;
    if (launch(k_rank_normalize, dim3((unsigned)m), dim3(EPX_RD_THREADS), lds, 0, a)) return -1;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(rank_out, rd, total * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(z_out, zd, total * 8, hipMemcpyDeviceToHost));
    return 0;
}

int epx_newgroup_latents(int device, int model, int D, uint64_t seed, int32_t label, long long t0, long long nt, int R,
                         double *out) {
    DeviceGuard guard;
    if (need_device(device)) return -1;
    const char *who = "epx_newgroup_latents";
    if (model < EPX_M1B_SG || model > EPX_M5A_SG) return fail("%s: unknown model %d", who, model);
    if (D < 1 || D > EPX_PR_DMAX) return fail("%s: D = %d columns, between 1 and %d", who, D, (int)EPX_PR_DMAX);
    if (label < 0) return fail("%s: label %d is negative", who, (int)label);
    if (R < 1 || R > EPX_NGP_RMAX) return fail("%s: R must be in 1..%d (got %d)", who, (int)EPX_NGP_RMAX, R);
    if (t0 < 0 || nt < 0 || t0 > (1ll << 32) || nt > (1ll << 32) || t0 + nt > (1ll << 32))
        return fail("%s: pooled draws [%lld,%lld) outside [0,2^32)", who, t0, t0 + nt);
    if (nt == 0) return 0;
    if (!out) return fail("%s: out is required", who);
    const int b = model % 5, E = b == EPX_M1B_SG ? 1 : 1 + D;
    const size_t total = (size_t)nt * R * E;
    DevBuf<double> od;
    HIPCHK(od.alloc(total));
    const long long blocks = (nt * R * ((E + 1) / 2) + 255) / 256;
    hipLaunchKernelGGL(k_newgroup_latents, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, 0, seed,
                       (int)label, t0, nt, R, E, b == EPX_M5B_SG ? 1 : 0, od);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, od, total * 8, hipMemcpyDeviceToHost));
    return 0;
}

int epx_rng_probe(int device, uint64_t seed, int chain, uint32_t t, uint32_t kind, uint32_t a, uint32_t b,
                  double *out4) {
    DeviceGuard guard;
    if (need_device(device)) return -1;
    DevBuf<double> od;
    HIPCHK(od.alloc(4));
    hipLaunchKernelGGL(k_rng_probe, dim3(1), dim3(64), 0, 0, seed, chain, t, kind, a, b, od);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out4, od, 32, hipMemcpyDeviceToHost));
    return 0;
}

int epx_math_probe(int device, int kind, long long n, const double *a, const double *b, double *out) {
    DeviceGuard guard;
    if (need_device(device)) return -1;
    if (kind < 0 || kind >= EPX_MP_COUNT) return fail("epx_math_probe: unknown kind %d", kind);
    if (n < 0) return fail("epx_math_probe: n = %lld elements", n);
    if (n == 0) return 0;
    if (!a || !b || !out) return fail("epx_math_probe: a, b and out are required");
    DevBuf<double> ab, od;
    HIPCHK(ab.alloc((size_t)n * 2));
    HIPCHK(od.alloc((size_t)n * 4));
    double *ad = ab, *bd = ad + n;
    HIPCHK(hipMemcpy(ad, a, (size_t)n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(bd, b, (size_t)n * 8, hipMemcpyHostToDevice));
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_math_probe, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, 0, kind, n, ad, bd, od);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, od, (size_t)n * 4 * 8, hipMemcpyDeviceToHost));
    return 0;
}
