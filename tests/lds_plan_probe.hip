// Test helper: everything the library's LDS planning functions decide, over a sweep of shapes (links libepx.so).
// tests/golden/lds_plan.txt is this program's output with the library as it stood before the record sizes moved into
// csrc/nuts_geometry.h; test_lds_plan_is_unchanged (test_tree_endings_cases.py) compares line for line.
//
// Forms: layout 1 (nuts_lds_layout, wpc 1, cpb 1..4), layout 2 (wpc 4, cpb 1; Gaussian family or not; one group per site,
// or grp with ngmax in {1, 5, 40}), the row-wave / state-wave kernels (nuts_duo_lds_layout) (cpb, rw) = (4, 1), (4, 4), (1, 2).
// Shapes: (P, d) below, dp in {4, 8, 16, 32}, n_max in {1, 16, 48, 500, 2048, the largest whose plan still fits 160 KB},
// max_depth in {1, 2, 3, 4, 10, 12}.
//   L lines   every form x (P, d) x dp at the largest n_max, max_depth 10: each record size at each of its arguments
//   M lines   every form x n_max x max_depth at (P, d, dp) = (51, 34, 16), (99, 66, 32): where Omega, the tree stack, its
//             lowest levels and the speculative kernel's records go in and out of LDS (the kernels these plans select
//             are run, one row below and at every such boundary, from the table tests/resident_edge_cases.py)
//   ALL line  count and FNV-1a hash of the lines of the WHOLE cross product form x (P, d) x dp x n_max x max_depth
//   S lines   nuts_stream_lds_bytes: nv in {1, 2, 7}, resident (dpb 16, 32) and streaming (dpb 64, 128)
// A line: tag form wpc cpb rw grp ngmax gauss | P d dp n_max max_depth | n_max off_y off_xch off_gl off_Om off_tail off_slot
// off_flag off_spec off_scr off_stack off_piece slot_doubles scr_doubles stack_ps stack_lds_levels stack_in_lds om_in_lds
// duo_rw cpb lds_bytes | return value
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../ep-stan_amd/csrc/epx_kernels.h"

struct Form { const char *name; int duo, wpc, cpb, rw, grp, ngmax, gauss; };
static const Form FORMS[] = {
    {"l1", 0, 1, 1, 0, 0, 0, 0}, {"l1", 0, 1, 2, 0, 0, 0, 0}, {"l1", 0, 1, 3, 0, 0, 0, 0}, {"l1", 0, 1, 4, 0, 0, 0, 0},
    {"l2", 0, 4, 1, 0, 0, 0, 0}, {"l2", 0, 4, 1, 0, 0, 0, 1},
    {"l2", 0, 4, 1, 0, 1, 1, 0}, {"l2", 0, 4, 1, 0, 1, 5, 0}, {"l2", 0, 4, 1, 0, 1, 40, 0},
    {"l2", 0, 4, 1, 0, 1, 1, 1}, {"l2", 0, 4, 1, 0, 1, 5, 1}, {"l2", 0, 4, 1, 0, 1, 40, 1},
    {"duo", 1, 0, 4, 1, 0, 0, 0}, {"duo", 1, 0, 4, 4, 0, 0, 0}, {"duo", 1, 0, 1, 2, 0, 0, 0},
};
// sampled coordinates and shared parameters of sites of the model family: m1b D = 1 | m1a D = 32 | m4b D = 16 | m4a D = 20 |
// m1b D = 63 | m4b D = 32 | m1b D = 126 -- one and two registers per lane at their edges, d below, at and above 64
static const int SHAPES[][2] = {{3, 2}, {35, 34}, {51, 34}, {64, 43}, {65, 64}, {99, 66}, {128, 127}};
static const int DPS[] = {4, 8, 16, 32}, NMAX[] = {1, 16, 48, 500, 2048, -1}, DEPTHS[] = {1, 2, 3, 4, 10, 12};
static const size_t CAP = 160 * 1024;

static size_t plan(const Form &f, int P, int d, int dp, int n_max, int md, epx::NutsArgs &a) {
    memset(&a, 0, sizeof a);
    a.P = P; a.d = d; a.chains = 4; a.max_depth = md; a.cpb = f.cpb; a.grp = f.grp; a.ngmax = f.ngmax; a.gauss = f.gauss;
    return f.duo ? epx::nuts_duo_lds_layout(a, f.cpb, f.rw, dp, n_max) : epx::nuts_lds_layout(a, f.wpc, dp, n_max);
}

// the largest n_max whose plan fits the LDS (0: none does)
static int largest(const Form &f, int P, int d, int dp, int md) {
    epx::NutsArgs a;
    for (int n = (int)(CAP / (dp * 8)) + 1; n >= 1; --n)
        if (plan(f, P, d, dp, n, md, a) <= CAP) return n;
    return 0;
}

static int line(char *buf, size_t len, const char *tag, const Form &f, int P, int d, int dp, int n_max, int md) {
    epx::NutsArgs a;
    const size_t r = plan(f, P, d, dp, n_max, md, a);
    return snprintf(buf, len, "%s %s %d %d %d %d %d %d | %d %d %d %d %d | %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d | %zu\n",
                    tag, f.name, f.wpc, f.cpb, f.rw, f.grp, f.ngmax, f.gauss, P, d, dp, n_max, md,
                    a.n_max, a.off_y, a.off_xch, a.off_gl, a.off_Om, a.off_tail, a.off_slot, a.off_flag, a.off_spec, a.off_scr,
                    a.off_stack, a.off_piece, a.slot_doubles, a.scr_doubles, a.stack_ps, a.stack_lds_levels, a.stack_in_lds,
                    a.om_in_lds, a.duo_rw, a.cpb, a.lds_bytes, r);
}

int main() {
    char buf[512];
    for (const Form &f : FORMS)
        for (const auto &s : SHAPES)
            for (int dp : DPS) {
                line(buf, sizeof buf, "L", f, s[0], s[1], dp, largest(f, s[0], s[1], dp, 10), 10);
                fputs(buf, stdout);
            }
    const int tested[2][3] = {{51, 34, 16}, {99, 66, 32}};
    for (const Form &f : FORMS)
        for (const auto &t : tested)
            for (int md : DEPTHS)
                for (int n_max : NMAX) {
                    line(buf, sizeof buf, "M", f, t[0], t[1], t[2], n_max > 0 ? n_max : largest(f, t[0], t[1], t[2], md), md);
                    fputs(buf, stdout);
                }
    uint64_t h = 1469598103934665603ull;
    long count = 0;
    for (const Form &f : FORMS)
        for (const auto &s : SHAPES)
            for (int dp : DPS)
                for (int md : DEPTHS)
                    for (int n_max : NMAX) {
                        const int len = line(buf, sizeof buf, "A", f, s[0], s[1], dp, n_max > 0 ? n_max : largest(f, s[0], s[1], dp, md), md);
                        for (int i = 0; i < len; ++i) { h ^= (unsigned char)buf[i]; h *= 1099511628211ull; }
                        ++count;
                    }
    printf("ALL %ld %016llx\n", count, (unsigned long long)h);
    // streaming sampler: nv, dpb, d, ngmax, ntmax, rows kept in LDS (resident variant), gauss -> bytes
    const int nvd[3][2] = {{1, 34}, {2, 66}, {7, 130}};
    for (const auto &v : nvd)
        for (int dpb : {16, 32, 64, 128})
            for (int ngmax : {1, 5, 40})
                for (int ntmax : {1, 40, 700})
                    for (int alt = 0; alt < 2; ++alt) {
                        const bool res = dpb <= 32;
                        const int nmax_res = res ? (alt ? 500 : 48) : 0, gauss = res ? 0 : alt;
                        printf("S %d %d %d %d %d %d %d | %zu\n", v[0], dpb, v[1], ngmax, ntmax, nmax_res, gauss,
                               epx::nuts_stream_lds_bytes(v[0], dpb, v[1], ngmax, ntmax, nmax_res, gauss));
                    }
    return 0;
}
