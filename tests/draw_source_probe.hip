// Test helper: the pure front matter of the entries that post-process draws (csrc/epx_draws.h) on a context whose plain
// fields are filled by hand.  No HIP call is made: the context owns no stream, event or device array.
// usage: draw_source_probe source WHO K P s_chains s_nkeep drawn_k0 drawn_count has_draws k0 count inject S chains
//            (inject: 1 = the caller passes draws; chains: -1 = the entry takes none)
//            ->  "ok S chains at need"  |  "refused <message>"
//        draw_source_probe layout model gauss D d groups name...
//            (model: the b-model id the context keeps; groups: "-" or the groups per site, "1,3,2")
//            ->  one line "ok k L off[0] ... off[n_names]" for the largest site (k = -1) and for every site k,
//                or "refused <message>"
// (links libepx.so for epx_fail / epx_last_error)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../ep-stan_amd/csrc/epx_draws.h"

int main(int argc, char **argv) {
    epx_ctx c;
    if (argc == 15 && !strcmp(argv[1], "source")) {
        int v[12];
        for (int i = 0; i < 12; ++i) v[i] = atoi(argv[3 + i]);
        c.K = v[0]; c.P = v[1]; c.s_chains = v[2]; c.s_nkeep = v[3]; c.drawn_k0 = v[4]; c.drawn_count = v[5];
        static double fake[1];
        if (v[6]) c.draws.p = fake;                      // (only compared with NULL; cleared before the context goes)
        const int chains = v[11];
        epx::DrawSource src;
        const int rc = epx::draw_source(&c, argv[2], v[7], v[8], v[9] ? fake : nullptr, v[10], chains < 0 ? nullptr : &chains, &src);
        c.draws.p = nullptr;
        if (rc) printf("refused %s\n", epx_last_error());
        else printf("ok %d %d %zu %zu\n", src.S, src.chains, src.at, src.need);
        return 0;
    }
    if (argc >= 8 && !strcmp(argv[1], "layout")) {
        c.model = atoi(argv[2]); c.gauss = atoi(argv[3]); c.D = atoi(argv[4]); c.d = atoi(argv[5]);
        c.K = c.ng_max = 1;
        if (strcmp(argv[6], "-")) {                      // groups per site, as ctx_create keeps them
            c.multi = 1; c.K = 0;
            for (char *tok = strtok(argv[6], ","); tok; tok = strtok(nullptr, ",")) {
                c.g_cnt.push_back(atoi(tok)); ++c.K;
                if (c.g_cnt.back() > c.ng_max) c.ng_max = c.g_cnt.back();
            }
        }
        const int n_names = argc - 7;
        if (n_names > epx::EPX_NM_MAX_REQ) return 2;
        int32_t names[epx::EPX_NM_MAX_REQ];
        for (int i = 0; i < n_names; ++i) names[i] = atoi(argv[7 + i]);
        // k = -1: the row of the per-site entries (the context's largest site); k >= 0: of a pool that starts at site k
        for (int k = -1; k < c.K; ++k) {
            epx::NamedArgs a;
            if (epx::named_layout(&c, names, n_names, k < 0 ? c.ng_max : c.multi ? c.g_cnt[k] : 1, a)) {
                printf("refused %s\n", epx_last_error());
                return 0;
            }
            printf("ok %d %d", k, a.L);
            for (int i = 0; i <= n_names; ++i) printf(" %d", a.off[i]);
            printf("\n");
        }
        return 0;
    }
    return 2;
}
