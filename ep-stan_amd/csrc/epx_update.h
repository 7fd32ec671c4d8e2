// Private to libepx.so (host only, epx_api.hip alone includes it), the counterpart of epx_draws.h: what the update stage decides
// without a HIP call -- where the dense kernels (dense.hip) work, and the statistics block of epx_update_trial.
#pragma once
#include <cmath>

#include "epx_ctx.h"

namespace epx {

// A block of a dense kernel at dimension d works on two d x ld matrices and four vectors of ld doubles: in dynamic LDS while
// that leaves 1 KB of the CU's LDS to the kernels' static arrays (d <= 99: 159 984 B), else in its slot of a global workspace.
struct DensePlan {
    int ld;                    // leading dimension of the work matrices
    size_t slot;               // doubles per block
    bool in_lds;
    size_t lds_bytes;          // dynamic LDS of the launch (0 with the workspace)
    explicit DensePlan(int d) : ld(d | 1), slot(2 * (size_t)d * ld + 4 * (size_t)ld), in_lds(slot * 8 + 1024 <= lds_capacity()),
                                lds_bytes(in_lds ? slot * 8 : 0) {}
    size_t ws_doubles(int nblocks) const { return in_lds ? 0 : slot * (size_t)nblocks; }
};

// Room behind the packed sums (c->packed) for what rides on the same all-reduce: up to STAT_CAP sums, up to STAT_CAP maxima for
// each of up to 120 ranks, and from TRIAL_FLAGS_AT on the trial's [global_pd, all cavities pd, first failing site].
enum { STAT_CAP = 8, PACKED_EXTRA = 1024, TRIAL_FLAGS_AT = PACKED_EXTRA - 3 };

// The statistics block of one epx_update_trial, offsets in doubles from the end of the packed sums: sums in front, then n_max
// slots per rank for its maxima (the others' stay zero: the sum over ranks is an all-gather, the maximum is taken on the host).
struct TrialStats {
    int n_sum = 0, n_max = 0, ranks = 1, rank = 0;

    int count() const { return n_sum + n_max * ranks; }                 // doubles that travel
    size_t maxima_at(int r) const { return n_sum + (size_t)r * n_max; }
    // this rank's values into a zeroed block of count() doubles
    void pack(const double *stat_sum, const double *stat_max, double *block) const {
        for (int i = 0; i < n_sum; ++i) block[i] = stat_sum[i];
        for (int i = 0; i < n_max; ++i) block[maxima_at(rank) + i] = stat_max[i];
    }
    // the reduced block: sums as they are, maxima over the rank slots in rank order
    void unpack(const double *block, double *stat_sum, double *stat_max) const {
        for (int i = 0; i < n_sum; ++i) stat_sum[i] = block[i];
        for (int i = 0; i < n_max; ++i) stat_max[i] = block[maxima_at(0) + i];
        for (int r = 1; r < ranks; ++r)
            for (int i = 0; i < n_max; ++i) stat_max[i] = std::fmax(stat_max[i], block[maxima_at(r) + i]);
    }
    // k_trial_flags leaves the first failing site as a double, 1e17 or more when every site passed
    static int64_t first_bad(double v) { return v >= 1e17 ? -1 : (int64_t)v; }
};

// Refuses, or lays the block out for `ranks` ranks of which this one is `rank`.
inline int trial_stats(int n_sum, int n_max, int ranks, int rank, TrialStats *st) {
    if (n_sum < 0 || n_sum > STAT_CAP || n_max < 0 || n_max > STAT_CAP) return fail("at most %d statistics of a kind", (int)STAT_CAP);
    *st = {n_sum, n_max, ranks, rank};
    if (st->count() + 3 > PACKED_EXTRA) return fail("too many ranks (%d) for the statistics block", ranks);
    return 0;
}

}  // namespace epx
