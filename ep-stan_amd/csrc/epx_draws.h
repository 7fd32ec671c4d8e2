// Private to libepx.so (host only): what every entry point that post-processes draws has in front of its kernel --
// epx_named_moments, epx_named_order_stats, epx_pooled_count_pass, epx_predict, epx_predict_order_stats,
// epx_predict_new_group, epx_loo, epx_ppc, epx_site_evidence, epx_draw_diagnostics, epx_draw_rank_diagnostics and
// epx_pooled_moments.  The draws are those the last sampling call left in c->draws, or `theta` (count, S, P) of the caller,
// copied to c->inj.  Behind them: the ranks, padding and LDS budget of the entries that sort keys in LDS, and what the
// predictive entries (epx_predict, epx_predict_order_stats, epx_predict_new_group, epx_loo, epx_ppc; epx_site_evidence for
// its work items) share in front of the row-tile walk of predict_tile.h.
// Order of refusals in an entry: its own arguments (check_walk_columns, check_rank_count, check_ctx_rows); for the named
// entries the name list, then every name in turn; the draw source (draw_source: S, chains, "no draws yet", the sites
// drawn); whatever the entry derives from S (fill_ranks, the LDS limits; epx_loo has check_ctx_rows here); and only then
// the first copy (upload_draws), behind a StreamSync (epx_ctx.h) -- from there on every exit has synchronised c->stream,
// because the queued copies read the caller's memory; the kernels go out behind it too (launch, epx_ctx.h).  A refusal
// writes nothing to the caller's outputs.
#pragma once
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "epx_ctx.h"
#include "epx_kernels.h"

namespace epx {

struct DrawSource {
    int S = 0, chains = 0;           // draws per site; chains they came from (an entry that passed `chains`)
    const double *theta = nullptr;   // the caller's draws, or NULL: c->draws + at
    size_t at = 0, need = 0;         // first double of site k0 in c->draws; doubles of theta
};

// Pure (no HIP call): refuses, or says how many draws per site the call has and where they are.  chains: NULL, or the
// chains of injected draws (epx_draw_diagnostics, epx_site_evidence); draws of the sampler come in c->s_chains chains.
inline int draw_source(const epx_ctx *c, const char *who, int k0, int count, const double *theta, int S, const int *chains,
                       DrawSource *src) {
    src->theta = theta;
    if (theta) {
        if (S < 1) return fail("%s: S = %d draws", who, S);
        if (chains) {
            if (*chains < 1 || *chains > EPX_DG_MAX_CHAINS)
                return fail("%s: chains must be in 1..%d (got %d)", who, (int)EPX_DG_MAX_CHAINS, *chains);
            if (S % *chains != 0) return fail("%s: S = %d draws are no multiple of chains = %d", who, S, *chains);
            src->chains = *chains;
        }
    } else {
        S = c->s_chains * c->s_nkeep;
        if (!c->draws || S < 1 || c->drawn_count < 1) return fail("no draws yet");
        if (k0 < c->drawn_k0 || k0 + count > c->drawn_k0 + c->drawn_count)
            return fail("%s: sites [%d,%d) asked, the last sampling call left draws of sites [%d,%d) only", who,
                        k0, k0 + count, c->drawn_k0, c->drawn_k0 + c->drawn_count);
        src->chains = c->s_chains;
    }
    src->S = S;
    src->at = (size_t)k0 * S * c->P;
    src->need = (size_t)count * S * c->P;
    return 0;
}

// The device pointer of a source: injected draws are queued for copy into c->inj (grown), on c->stream.
inline int upload_draws(epx_ctx *c, const DrawSource &src, const double **draws) {
    if (src.theta) {
        HIPCHK(c->inj.grow(src.need));
        HIPCHK(hipMemcpyAsync(c->inj, src.theta, src.need * 8, hipMemcpyHostToDevice, c->stream));
    }
    *draws = src.theta ? c->inj : c->draws + src.at;
    return 0;
}

// The sites' group prefix on the device as the argument structs take it: NULL where every site has one group
inline const int *site_g0(const epx_ctx *c) { return c->multi ? (const int *)c->site_g0_d : nullptr; }

// The ranks of the order-statistic entries: as arguments, in front of the draw source ...
inline int check_rank_count(const char *who, const int64_t *ranks, int n_ranks) {
    const bool ok = ranks && n_ranks >= 1 && n_ranks <= EPX_QT_MAX_RANKS;
    return ok ? 0 : fail("%s: between 1 and %d ranks (got %d)", who, (int)EPX_QT_MAX_RANKS, n_ranks);
}
// ... and behind it, against the S draws per site: ascending, distinct; rank[] as the kernels take it
inline int fill_ranks(const char *who, const int64_t *ranks, int n_ranks, int S, int (&rank)[EPX_QT_MAX_RANKS]) {
    for (int i = 0; i < n_ranks; ++i) {
        if (ranks[i] < 0 || ranks[i] >= S)
            return fail("%s: rank %lld outside [0, %d), the draws per site", who, (long long)ranks[i], S);
        if (i > 0 && ranks[i] <= ranks[i - 1]) return fail("%s: the ranks have to be ascending and distinct", who);
    }
    for (int i = 0; i < EPX_QT_MAX_RANKS; ++i) rank[i] = i < n_ranks ? (int)ranks[i] : 0;
    return 0;
}

// S keys padded to a power of two, at least 2, for the sort in LDS; lg: its logarithm
inline int pow2_pad(int S, int *lg = nullptr) {
    int npad = 2, l = 1;
    for (; npad < S; npad *= 2) ++l;
    if (lg) *lg = l;
    return npad;
}

// An LDS budget that a test and A/B knob of the environment (EPX_PO_LDS_BYTES, EPX_LOO_LDS_BYTES), read at every call, may
// lower: a value that is no whole non-negative number, or not below `bytes`, is ignored.  lowered stays empty, or is
// what a refusal says of the variable.
inline size_t lds_budget(const char *var, size_t bytes, std::string *lowered = nullptr) {
    const char *e = getenv(var);
    char *end = nullptr;
    const long long v = e ? strtoll(e, &end, 10) : -1;
    if (!e || end == e || *end != '\0' || v < 0 || (size_t)v >= bytes) return bytes;
    if (lowered) *lowered = std::string("; ") + var + " = " + e + " lowers the keys' budget";
    return (size_t)v;
}

// name, off and L of `a` for sites of ng groups: off[i] = first element of name i's block in a row of L elements
// (the slots behind n_names repeat L); model, D, d and gauss come from the context.
inline int named_layout(const epx_ctx *c, const int32_t *names, int n_names, int ng, NamedArgs &a) {
    a.n_names = n_names; a.off[0] = 0;
    for (int i = 0; i < EPX_NM_MAX_REQ; ++i) {
        const int n = i < n_names ? named_len(names[i], c->model, c->D, c->d, c->gauss, ng) : 0;
        if (n < 0) return fail("named parameter %d is not defined by this site model", (int)names[i]);
        a.name[i] = i < n_names ? names[i] : 0; a.off[i + 1] = a.off[i] + n;
    }
    a.L = a.off[n_names];
    return 0;
}

// Everything of the NamedArgs of a call over named parameters but `draws`, rows laid out for ng groups; pure.
inline int named_front(const epx_ctx *c, const char *who, int k0, int count, const int32_t *names, int n_names,
                       const double *theta, int S, int ng, NamedArgs &a, DrawSource *src) {
    if (!names || n_names < 1 || n_names > EPX_NM_MAX_REQ) return fail("%s: between 1 and %d names", who, (int)EPX_NM_MAX_REQ);
    a.model = c->model; a.D = c->D; a.d = c->d; a.gauss = c->gauss; a.P = c->P;
    a.ng_max = c->ng_max; a.k0 = k0; a.site_g0 = site_g0(c);
    a.draws = nullptr; a.mean = a.m2 = nullptr;
    if (named_layout(c, names, n_names, ng, a)) return -1;
    if (draw_source(c, who, k0, count, theta, S, nullptr, src)) return -1;
    a.S = src->S;
    return 0;
}

// ---- the predictive entries
inline PredictModel predict_model(const epx_ctx *c) {
    return PredictModel{c->model, c->D, c->d, c->gauss, c->P, (1 + c->D + 3) / 4 * 4};
}

// The size refusals: the walk's columns, and the context's own rows, which work items hold as ints (cut_ctx_rows)
inline int check_walk_columns(const epx_ctx *c, const char *who) {
    return c->D > EPX_PR_DMAX ? fail("%s: D = %d columns, at most %d", who, c->D, (int)EPX_PR_DMAX) : 0;
}
inline int check_ctx_rows(const epx_ctx *c, const char *who) {
    return c->N > 0x7fffffff ? fail("%s: %lld rows, at most 2^31 - 1", who, (long long)c->N) : 0;
}

// The walk bound to the model, S draws per site and the sites from k0 on; every pointer NULL: the entry sets draws, wg, X, ...
inline PredictArgs bind_walk(const epx_ctx *c, int k0, int S) {
    PredictArgs a = {};
    a.m = predict_model(c); a.S = S; a.k0 = k0; a.site_g0 = site_g0(c);
    return a;
}

// The first row of [0, n) whose response the family does not take, or -1.  Bernoulli: 0 or 1; Gaussian: anything, or
// with `finite` (a new group's joint term adds the rows' terms up) finite values only.
inline int64_t bad_response(const epx_ctx *c, const double *yn, int64_t n, bool finite) {
    for (int64_t i = 0; i < n; ++i)
        if (c->gauss ? finite && !std::isfinite(yn[i]) : (yn[i] != 0.0 && yn[i] != 1.0)) return i;
    return -1;
}

// Stable counting sort of the rows [lo, hi) by their group in [0, ng) (row_group NULL: all in group 0): the rows of
// group g, in their order, are perm[first[g]] .. perm[first[g + 1]], first[0] = lo.  Returns the first row whose group
// is out of range (nothing of perm is written then), or -1.
inline int64_t sort_rows_by_group(int64_t lo, int64_t hi, const int32_t *row_group, int ng, int *perm, std::vector<int> &first) {
    first.assign((size_t)ng + 1, 0);
    for (int64_t i = lo; i < hi; ++i) {
        const int g = row_group ? row_group[i] : 0;
        if (g < 0 || g >= ng) return i;
        ++first[(size_t)g + 1];
    }
    first[0] = (int)lo;
    for (int g = 0; g < ng; ++g) first[(size_t)g + 1] += first[g];
    std::vector<int> at(first.begin(), first.end() - 1);
    for (int64_t i = lo; i < hi; ++i) perm[at[row_group ? row_group[i] : 0]++] = (int)i;
    return -1;
}

// The limits of the new rows of the sites of a call (epx_predict, epx_predict_order_stats): refuses, or says how many
// rows there are
inline int new_row_count(const char *who, int k0, int count, const int64_t *row_lim, int64_t *n) {
    if (!row_lim) return fail("%s: row_lim is required", who);
    if (row_lim[0] != 0) return fail("%s: row_lim has to start at 0 (it starts at %lld)", who, (long long)row_lim[0]);
    for (int j = 0; j < count; ++j)
        if (row_lim[j + 1] < row_lim[j])
            return fail("%s: row_lim has to be non-decreasing (site %d: [%lld,%lld))", who, k0 + j,
                        (long long)row_lim[j], (long long)row_lim[j + 1]);
    *n = row_lim[count];
    if (*n > 0x7fffffff) return fail("%s: %lld rows in one call, at most 2^31 - 1", who, (long long)*n);
    return 0;
}

// How new rows are cut into work items, stated once: the rows sorted by (site, group), stable -- perm[sorted position] =
// row (perm: n ints) -- then items of at most `item` rows of ONE (site, group), in that order
inline int cut_new_rows(const epx_ctx *c, const char *who, int k0, int count, const int64_t *row_lim, const int32_t *row_group,
                        int item, int *perm, std::vector<PredictWg> &wg) {
    std::vector<int> first;
    for (int j = 0; j < count; ++j) {
        const int ng = c->multi ? c->g_cnt[k0 + j] : 1;
        if (const int64_t i = sort_rows_by_group(row_lim[j], row_lim[j + 1], row_group, ng, perm, first); i >= 0)
            return fail("%s: row %lld: group %d outside the %d group(s) of site %d", who, (long long)i,
                        row_group ? (int)row_group[i] : 0, ng, k0 + j);
        for (int g = 0; g < ng; ++g)
            for (int r = first[g]; r < first[g + 1]; r += item)
                wg.push_back(PredictWg{j, g, r, first[g + 1] - r < item ? first[g + 1] - r : item});
    }
    return 0;
}

// How the context's OWN rows are cut into work items, stated once (epx_loo, epx_ppc, epx_site_evidence; behind
// check_ctx_rows): the sites of the range in order, each site's groups in order, items {site of the call, group, first row,
// rows} of at most `item` rows; item = 0: every group whole, one item each.  site_first: the first item of every site.
inline void cut_ctx_rows(const epx_ctx *c, int k0, int count, int item, std::vector<PredictWg> &wg,
                         std::vector<int> *site_first = nullptr) {
    if (site_first) site_first->assign((size_t)count + 1, 0);
    for (int j = 0; j < count; ++j) {
        const int k = k0 + j, ng = c->multi ? c->g_cnt[k] : 1;
        const int64_t *lim = c->multi ? c->g_lim.data() + c->site_g0[k] : c->k_lim.data() + k;
        for (int g = 0; g < ng; ++g) {
            const int64_t lo = lim[g], hi = lim[g + 1];
            if (!item) wg.push_back(PredictWg{j, g, (int)lo, (int)(hi - lo)});
            for (int64_t r = lo; item && r < hi; r += item)
                wg.push_back(PredictWg{j, g, (int)r, (int)(hi - r < item ? hi - r : item)});
        }
        if (site_first) (*site_first)[(size_t)j + 1] = (int)wg.size();
    }
}

// Queues the copy of the work items to wg_d (4 ints each); behind a StreamSync declared behind `wg`
inline int upload_items(epx_ctx *c, const std::vector<PredictWg> &wg, int *wg_d, const PredictWg **items) {
    static_assert(sizeof(PredictWg) == 4 * sizeof(int), "PredictWg is four ints");
    HIPCHK(hipMemcpyAsync(wg_d, wg.data(), wg.size() * sizeof(PredictWg), hipMemcpyHostToDevice, c->stream));
    *items = reinterpret_cast<const PredictWg *>(wg_d);
    return 0;
}

// Queues the copies of the n new rows, their responses (if any) and the sort's perm; behind a StreamSync
inline int queue_new_rows(epx_ctx *c, size_t n, const double *Xn, const double *yn, const int *perm, double *X_d, double *y_d,
                          int *perm_d) {
    HIPCHK(hipMemcpyAsync(X_d, Xn, n * c->D * 8, hipMemcpyHostToDevice, c->stream));
    if (yn) HIPCHK(hipMemcpyAsync(y_d, yn, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(perm_d, perm, n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    return 0;
}

// The grid of a kernel whose workgroups walk their items: every item its own workgroup up to per_cu per compute unit
inline unsigned walk_grid(const epx_ctx *c, size_t items, int per_cu) {
    const size_t cap = (size_t)(c->n_cu > 0 ? c->n_cu : 256) * per_cu;
    return (unsigned)(items < cap ? items : cap);
}

}  // namespace epx
