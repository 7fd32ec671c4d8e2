// Test helper: the sizes the library's own functions give the PSIS stage (csrc/psis.h) and the first S epx_psis_rows
// refuses (csrc/epx_api.hip: 16 rows' scratch against the LDS capacity less 1 KiB, or more fit points than PSIS_FIT_MAX).
// usage: psis_plan_probe cap            ->  lds_capacity() PSIS_MIN_TAIL PSIS_FIT_MAX
//        psis_plan_probe sizes S ...    ->  one line per S: S M m tail_pad cand_cap scratch_doubles
//        psis_plan_probe first          ->  the first S that is refused: S M m scratch_doubles, then the same for S - 1
// (host code only; links libepx.so as the other probes do)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../ep-stan_amd/csrc/epx_kernels.h"
#include "../ep-stan_amd/csrc/psis.h"

static bool refused(int S) {
    const int M = epx::psis_tail_length(S);
    return epx::psis_fit_points(M) > epx::PSIS_FIT_MAX ||
           (size_t)16 * epx::psis_scratch_doubles(M) * 8 > epx::lds_capacity() - 1024;
}

static void line(int S) {
    const int M = epx::psis_tail_length(S);
    printf("%d %d %d %d %d %d\n", S, M, epx::psis_fit_points(M), epx::psis_tail_pad(M), epx::psis_cand_cap(M),
           epx::psis_scratch_doubles(M));
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "cap")) {
        printf("%zu %d %d\n", epx::lds_capacity(), (int)epx::PSIS_MIN_TAIL, (int)epx::PSIS_FIT_MAX);
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "sizes")) {
        for (int i = 2; i < argc; ++i) line(atoi(argv[i]));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "first")) {
        for (int S = 1; S < (1 << 24); ++S)
            if (refused(S)) {
                line(S);
                line(S - 1);
                return 0;
            }
        return 3;
    }
    return 2;
}
