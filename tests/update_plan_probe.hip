// Test helper: what the update stage decides without a HIP call (csrc/epx_update.h).  No HIP call is made.
// usage: update_plan_probe plan D NBLOCKS
//            ->  "ld slot in_lds lds_bytes ws_doubles"
//        update_plan_probe stats N_SUM N_MAX RANKS RANK
//            ->  "ok count maxima_at(RANK) TRIAL_FLAGS_AT"  |  "refused <message>"
//        update_plan_probe pack N_SUM N_MAX RANKS RANK value...          (N_SUM sums, then N_MAX maxima)
//            ->  the block of count doubles, this rank's values in a zeroed block
//        update_plan_probe unpack N_SUM N_MAX RANKS value...             (the reduced block: count doubles)
//            ->  N_SUM sums, then N_MAX maxima
//        update_plan_probe first_bad VALUE
//            ->  the site index, or -1
// Doubles go in through strtod and come out as %a: every bit, the sign of a zero included.
// (links libepx.so for epx_fail / epx_last_error)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../ep-stan_amd/csrc/epx_update.h"

static void print_doubles(const double *v, size_t n) {
    for (size_t i = 0; i < n; ++i) printf("%s%a", i ? " " : "", v[i]);
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "plan")) {
        const epx::DensePlan p(atoi(argv[2]));
        printf("%d %zu %d %zu %zu\n", p.ld, p.slot, (int)p.in_lds, p.lds_bytes, p.ws_doubles(atoi(argv[3])));
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "first_bad")) {
        printf("%lld\n", (long long)epx::TrialStats::first_bad(strtod(argv[2], nullptr)));
        return 0;
    }
    const bool stats = argc == 6 && !strcmp(argv[1], "stats"), pack = argc >= 6 && !strcmp(argv[1], "pack"),
               unpack = argc >= 5 && !strcmp(argv[1], "unpack");
    if (!stats && !pack && !unpack) return 2;
    epx::TrialStats st;
    if (epx::trial_stats(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), unpack ? 0 : atoi(argv[5]), &st)) {
        printf("refused %s\n", epx_last_error());
        return 0;
    }
    if (stats) {
        printf("ok %d %zu %zu\n", st.count(), st.maxima_at(st.rank), (size_t)epx::TRIAL_FLAGS_AT);
        return 0;
    }
    std::vector<double> in;
    for (int i = unpack ? 5 : 6; i < argc; ++i) in.push_back(strtod(argv[i], nullptr));
    if (pack) {
        if ((int)in.size() != st.n_sum + st.n_max || st.rank < 0 || st.rank >= st.ranks) return 2;
        std::vector<double> block((size_t)st.count(), 0.0);
        st.pack(in.data(), in.data() + st.n_sum, block.data());
        print_doubles(block.data(), block.size());
    } else {
        if ((int)in.size() != st.count()) return 2;
        std::vector<double> out((size_t)st.n_sum + st.n_max, 0.0);
        st.unpack(in.data(), out.data(), out.data() + st.n_sum);
        print_doubles(out.data(), out.size());
    }
    return 0;
}
