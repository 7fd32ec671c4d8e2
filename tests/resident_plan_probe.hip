// Test helper: what the library's own LDS planning decides for the resident sampler kernels (links libepx.so): the
// fields of NutsArgs that launch_wpc (csrc/nuts.hip) and launch_duo_one (csrc/nuts_duo.hip) switch on.
// usage: resident_plan_probe cap     ->  the LDS capacity the planner compares with
//        resident_plan_probe plan    ->  reads tuples from standard input, one per line:
//                                          form wpc cpb rw grp ngmax gauss P d dp n_max max_depth
//                                        form 0: nuts_lds_layout(a, wpc, dp, n_max) with a.cpb = cpb
//                                        form 1: nuts_duo_lds_layout(a, cpb, rw, dp, n_max)
//                                      and prints one line per tuple:
//                                          om_in_lds stack_in_lds stack_lds_levels off_spec off_tail-bytes lds_bytes return
//                                          nuts_duo_has team_tiles_per_wave npad tail-columns
// The last three are read off the plan itself: the row team's rows are 64 * team_tiles_per_wave, laid out in front of
// off_Om; the cavity precision of the row-wave kernels takes npad * min(d, 64) * 16 bytes between off_Om and off_tail,
// and the tail record behind it holds the columns beyond 64 (2 * (2 npad + 2) doubles when NV = 2).
#include <cstdio>
#include <cstring>

#include "../ep-stan_amd/csrc/epx_kernels.h"

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "cap")) {
        printf("%zu\n", epx::lds_capacity());
        return 0;
    }
    if (argc != 2 || strcmp(argv[1], "plan")) return 2;
    int form, wpc, cpb, rw, grp, ngmax, gauss, P, d, dp, n_max, md;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d", &form, &wpc, &cpb, &rw, &grp, &ngmax, &gauss, &P, &d, &dp, &n_max, &md) == 12) {
        epx::NutsArgs a;
        memset(&a, 0, sizeof a);
        a.P = P; a.d = d; a.chains = 4; a.max_depth = md; a.cpb = cpb; a.grp = grp; a.ngmax = ngmax; a.gauss = gauss;
        const size_t r = form ? epx::nuts_duo_lds_layout(a, cpb, rw, dp, n_max) : epx::nuts_lds_layout(a, wpc, dp, n_max);
        const int nv = (P + 63) / 64;
        const bool team = form && epx::duo_team(cpb, rw);
        const int dm = d < 64 ? d : 64;
        const int tpw = team ? a.off_Om / (dp * 8) / 64 : 0;
        const int npad = form && !team ? (a.off_tail - a.off_Om) / (dm * 16) : 0;
        printf("%d %d %d %d %d %d %zu %d %d %d %d\n", a.om_in_lds, a.stack_in_lds, a.stack_lds_levels, a.off_spec,
               form ? a.off_slot - a.off_tail : 0, a.lds_bytes, r, form ? (int)epx::nuts_duo_has(cpb, rw, dp, nv) : 1, tpw, npad,
               form && d > 64 ? d - 64 : 0);
    }
    return 0;
}
