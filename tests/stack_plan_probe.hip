// Test helper: where the library's own LDS planning puts the tree stack of a resident sampler launch.
// usage: stack_plan_probe P d dp n_max max_depth   ->   one line per layout (1, 5, 7):
//   layout stack_in_lds stack_lds_levels lds_bytes
// (the calls plan_sampler of csrc/epx_api.hip makes for these layouts; links libepx.so)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../ep-stan_amd/csrc/epx_kernels.h"

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    const int P = atoi(argv[1]), d = atoi(argv[2]), dp = atoi(argv[3]), n_max = atoi(argv[4]), md = atoi(argv[5]);
    const int forms[3][3] = {{1, 4, 0}, {5, 4, 1}, {7, 4, 4}};           // layout, chains per workgroup, row waves
    for (int i = 0; i < 3; ++i) {
        epx::NutsArgs a;
        memset(&a, 0, sizeof a);
        a.P = P; a.d = d; a.chains = 4; a.max_depth = md; a.cpb = forms[i][1];
        const size_t lds = forms[i][0] == 1 ? epx::nuts_lds_layout(a, 1, dp, n_max)
                                            : epx::nuts_duo_lds_layout(a, forms[i][1], forms[i][2], dp, n_max);
        printf("%d %d %d %zu\n", forms[i][0], a.stack_in_lds, a.stack_lds_levels, lds);
    }
    return 0;
}
