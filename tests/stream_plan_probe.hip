// Test helper: the LDS bytes the library's own planning gives the streaming sampler (layout 3) and its resident
// variant (layout 4).
// usage: stream_plan_probe cap                                              ->  the LDS capacity the planner compares with
//        stream_plan_probe bytes nv dpb d ngmax ntmax nmax_res gauss ...    ->  one line per group of seven: the bytes
//        stream_plan_probe first nv dpb d ngmax gauss extra                 ->  the first tile count whose bytes + extra exceed
//                                                                               the capacity, the bytes one tile below, at it
// (nuts_stream_lds_bytes as plan_sampler of csrc/epx_api.hip calls it; links libepx.so)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../ep-stan_amd/csrc/epx_kernels.h"

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "cap")) {
        printf("%zu\n", epx::lds_capacity());
        return 0;
    }
    if (argc >= 9 && (argc - 2) % 7 == 0 && !strcmp(argv[1], "bytes")) {
        for (int i = 2; i < argc; i += 7)
            printf("%zu\n", epx::nuts_stream_lds_bytes(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]),
                                                       atoi(argv[i + 4]), atoi(argv[i + 5]), atoi(argv[i + 6])));
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "first")) {
        const int nv = atoi(argv[2]), dpb = atoi(argv[3]), d = atoi(argv[4]), ngmax = atoi(argv[5]), gauss = atoi(argv[6]);
        const size_t extra = (size_t)atol(argv[7]), cap = epx::lds_capacity();
        for (int nt = 1; nt < (1 << 20); ++nt) {
            const size_t b = epx::nuts_stream_lds_bytes(nv, dpb, d, ngmax, nt, 0, gauss);
            if (b + extra > cap) {
                printf("%d %zu %zu\n", nt, nt > 1 ? epx::nuts_stream_lds_bytes(nv, dpb, d, ngmax, nt - 1, 0, gauss) : 0, b);
                return 0;
            }
        }
        return 3;
    }
    return 2;
}
