// Test helper: the pure front matter of the entries that post-process draws (csrc/epx_draws.h) on a context whose plain
// fields are filled by hand.  No HIP call is made: the context owns no stream, event or device array.
// usage: draw_source_probe source WHO K P s_chains s_nkeep drawn_k0 drawn_count has_draws k0 count inject S chains
//            (inject: 1 = the caller passes draws; chains: -1 = the entry takes none)
//            ->  "ok S chains at need"  |  "refused <message>"
//        draw_source_probe layout model gauss D d groups name...
//            (model: the b-model id the context keeps; groups: "-" or the groups per site, "1,3,2")
//            ->  one line "ok k L off[0] ... off[n_names]" for the largest site (k = -1) and for every site k,
//                or "refused <message>"
//        draw_source_probe items rows k0 count item
//            (rows: the rows of every group, sites apart by "/": "3/0/16" has one group per site and no g_cnt, "9/8,7,9/10,6"
//            is multi-group; item: rows per work item, 0 = whole groups)
//            ->  one line "wg site group first rows" per work item, then "first" and the count + 1 entries of site_first
//        draw_source_probe ranks WHO S list
//            (list: "null", "none" for 0 ranks behind a pointer, or "0,4")
//            ->  "ok" and the EPX_QT_MAX_RANKS entries of rank[]  |  "refused <message>"
//        draw_source_probe pad S                  ->  "npad lg"
//        draw_source_probe budget VAR default     ->  "bytes|<what a refusal appends>"  (VAR read from the environment)
// (links libepx.so for epx_fail / epx_last_error)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../ep-stan_amd/csrc/epx_draws.h"

// "3,0,16" -> numbers
static std::vector<int64_t> numbers(const std::string &s) {
    std::vector<int64_t> v;
    for (size_t at = 0; at < s.size();) {
        const size_t end = s.find(',', at) == std::string::npos ? s.size() : s.find(',', at);
        v.push_back(atoll(s.substr(at, end - at).c_str()));
        at = end + 1;
    }
    return v;
}

int main(int argc, char **argv) {
    epx_ctx c;
    if (argc == 6 && !strcmp(argv[1], "items")) {
        // k_lim, g_cnt, g_lim and site_g0 as ctx_create keeps them (which refuses empty groups: here they are allowed)
        const std::string rows = argv[2];
        c.multi = rows.find(',') != std::string::npos;
        c.k_lim.push_back(0); c.g_lim.push_back(0); c.site_g0.push_back(0);
        for (size_t at = 0; at < rows.size();) {
            const size_t end = rows.find('/', at) == std::string::npos ? rows.size() : rows.find('/', at);
            const std::vector<int64_t> g = numbers(rows.substr(at, end - at));
            for (int64_t n : g) c.g_lim.push_back(c.g_lim.back() + n);
            c.g_cnt.push_back((int)g.size());
            c.site_g0.push_back(c.site_g0.back() + (int)g.size());
            c.k_lim.push_back(c.g_lim.back());
            at = end + 1;
        }
        c.K = (int)c.g_cnt.size(); c.N = c.k_lim.back();
        if (!c.multi) { c.g_cnt.clear(); c.g_lim.clear(); }
        const int k0 = atoi(argv[3]), count = atoi(argv[4]);
        std::vector<epx::PredictWg> wg;
        std::vector<int> site_first;
        epx::cut_ctx_rows(&c, k0, count, atoi(argv[5]), wg, &site_first);
        for (const epx::PredictWg &w : wg) printf("wg %d %d %d %d\n", w.site, w.group, w.first, w.rows);
        printf("first");
        for (int f : site_first) printf(" %d", f);
        printf("\n");
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "ranks")) {
        const std::vector<int64_t> list = strcmp(argv[4], "null") && strcmp(argv[4], "none") ? numbers(argv[4]) : std::vector<int64_t>();
        static const int64_t none[1] = {0};
        const int64_t *ranks = !strcmp(argv[4], "null") ? nullptr : list.empty() ? none : list.data();
        int rank[epx::EPX_QT_MAX_RANKS];
        if (epx::check_rank_count(argv[2], ranks, (int)list.size()) ||
            epx::fill_ranks(argv[2], ranks, (int)list.size(), atoi(argv[3]), rank)) {
            printf("refused %s\n", epx_last_error());
            return 0;
        }
        printf("ok");
        for (int r : rank) printf(" %d", r);
        printf("\n");
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "pad")) {
        int lg = 0;
        const int npad = epx::pow2_pad(atoi(argv[2]), &lg);
        printf("%d %d\n", npad, lg);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "budget")) {
        std::string lowered;
        const size_t bytes = epx::lds_budget(argv[2], (size_t)atoll(argv[3]), &lowered);
        printf("%zu|%s\n", bytes, lowered.c_str());
        return 0;
    }
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
