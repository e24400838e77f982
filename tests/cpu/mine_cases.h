// The specimine shapes of the plan tests, shared by the CPU simulation (tests/cpu/mine_plan_sim.cpp, which checks every
// output element against a full-matrix DP) and the sanitizer driver (tests/asan/mine_driver.cpp): queries of every
// state class, targets from empty to flanked copies, jobs of 0 to 300 targets that share ranges and span classes.
#ifndef SMX_TESTS_MINE_CASES_H
#define SMX_TESTS_MINE_CASES_H
#include <cstdio>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "mine_host.h"

namespace smx {

struct MineCase {
    std::string qbytes, tbytes;
    std::vector<uint64_t> qoff{0}, toff{0};
    std::vector<smx_mine_job> jobs;
    uint32_t nq() const { return (uint32_t)qoff.size() - 1; }
    uint32_t nt() const { return (uint32_t)toff.size() - 1; }
    std::string query(uint32_t q) const { return qbytes.substr(qoff[q], qoff[q + 1] - qoff[q]); }
    std::string target(uint32_t t) const { return tbytes.substr(toff[t], toff[t + 1] - toff[t]); }
    void add_query(const std::string &s) { qbytes += s; qoff.push_back(qbytes.size()); }
    void add_target(const std::string &s) { tbytes += s; toff.push_back(tbytes.size()); }
};

inline std::string mine_rand_seq(std::mt19937 &rng, int n) {
    std::string s(n, 'A');
    for (char &c : s) c = "ACGTN"[rng() % 5];
    return s;
}

inline std::string mine_mutate(std::mt19937 &rng, const std::string &s, int per_mille) {
    std::string out;
    for (char c : s) {
        const int r = (int)(rng() % 1000);
        if (r < per_mille) out.push_back("ACGT"[rng() % 4]);
        else if (r < 2 * per_mille) { out.push_back(c); out.push_back("ACGT"[rng() % 4]); }
        else if (r >= 3 * per_mille) out.push_back(c);
    }
    return out;
}

// query lengths: classes 1 (1, 63, 64), 2 (65, 128), 3 (129), 4 (257), 5 (513, 1024) and 0 (1025, 1100)
static const int kMineLens[11] = {1, 63, 64, 65, 128, 129, 257, 513, 1024, 1025, 1100};

inline MineCase mine_case(uint32_t seed) {
    std::mt19937 rng(seed);
    MineCase C;
    for (int m : kMineLens) C.add_query(mine_rand_seq(rng, m));
    for (int i = 0; i < 430; i++) {
        const std::string q = C.query((uint32_t)(i % 11));
        switch (i % 8) {
            case 0: C.add_target(mine_rand_seq(rng, 1 + (int)(rng() % 40)) + q + mine_rand_seq(rng, (int)(rng() % 40))); break;   // a flanked copy
            case 1: C.add_target(mine_mutate(rng, q, 15 + (int)(rng() % 60))); break;          // a mutated copy, now and then empty
            case 2: C.add_target(mine_rand_seq(rng, (int)q.size() / 3 + 40)); break;          // a stranger
            case 3: C.add_target(i % 16 == 3 ? "" : q.substr(q.size() / 4, q.size() / 2)); break;   // empty, or shorter than m - k
            case 4: C.add_target(mine_rand_seq(rng, 15)); break;
            case 5: C.add_target(mine_rand_seq(rng, 16)); break;
            case 6: C.add_target(mine_rand_seq(rng, 17)); break;
            default: C.add_target(q); break;
        }
    }
    C.jobs = {
        smx_mine_job{0, 11, 0, 300, 0.9},     // queries of every class over 300 targets (three chunks per record)
        smx_mine_job{0, 11, 0, 300, 0.0},     // the same target range again: outputs of its own
        smx_mine_job{2, 3, 300, 1, 1.0},      // one target
        smx_mine_job{5, 3, 301, 127, 0.9},
        smx_mine_job{8, 3, 100, 128, 0.0},    // inside the first job's targets
        smx_mine_job{0, 3, 50, 129, 1.0},
        smx_mine_job{3, 1, 7, 0, 0.9},        // no targets: no record, no output
        smx_mine_job{0, 0, 0, 10, 0.9},       // no queries: ten best identities that stay zero
        smx_mine_job{9, 2, 428, 2, 0.0},      // the generic class alone over the last targets
    };
    return C;
}

// the limit of query q in variant v: -1, 0, m / 10, above m, rotating with the query
inline std::vector<int32_t> mine_case_k(const MineCase &C, int variant) {
    std::vector<int32_t> k(C.nq());
    for (uint32_t q = 0; q < C.nq(); q++) {
        const int m = (int)(C.qoff[q + 1] - C.qoff[q]);
        const int kinds[4] = {-1, 0, m / 10, m + 5};
        k[q] = kinds[(q + (uint32_t)variant) % 4];
    }
    return k;
}

// HW distance by the O(nm) recurrence: the least last-row value over the columns 1..n; an empty target costs m
inline int mine_ref_hw(const std::string &p, const std::string &t) {
    const int m = (int)p.size(), n = (int)t.size();
    if (n == 0) return m;
    std::vector<int> col(m + 1);
    for (int i = 0; i <= m; i++) col[i] = i;
    int best = m;
    for (int j = 0; j < n; j++) {
        int diag = 0;
        for (int i = 1; i <= m; i++) {
            const int up = col[i - 1] + 1, left = col[i] + 1, sub = diag + (p[i - 1] == t[j] ? 0 : 1);
            diag = col[i];
            col[i] = std::min(std::min(up, left), sub);
        }
        best = std::min(best, col[m]);
    }
    return best;
}

struct MineCaseTotals {
    MineHostCounts H;
    long long plans = 0, compared = 0, mismatches = 0, within = 0, beyond = 0, best_set = 0, capped_plans = 0;
};

// Plans and runs the case in both modes for the four limit variants under `budget` (0: the production figure, 1: one
// slice of the generic class).  ref: distance of (query, target) without a limit, or null: then the best identities
// are checked against the twin's own distances alone.
inline void mine_case_run(const MineCase &C, int budget_kind, const std::map<std::pair<uint32_t, uint32_t>, int> *ref,
                          MineCaseTotals *totals) {
    MineCaseTotals &Tt = *totals;
    for (int variant = 0; variant < 4; variant++) {
        const std::vector<int32_t> k = mine_case_k(C, variant);
        MinePlan P;
        std::string why;
        uint64_t budget = CHUNK_SCRATCH_BYTES;
        if (budget_kind == 1) budget = chunk_slice_words(18) * 8;     // 1100 bases are 18 words
        if (mine_plan(C.qbytes.data(), C.qoff.data(), C.nq(), k.data(), C.tbytes.data(), C.toff.data(), C.nt(), C.jobs.data(),
                      (uint32_t)C.jobs.size(), budget, &P, &why) != SMX_OK)
            host_twin_fail(why.c_str());
        if (budget_kind == 1) {
            if (P.grid[0] != 1 || P.per_block[0] != P.chunks[0] || P.scratch_words != chunk_slice_words(P.words_max0))
                host_twin_fail("a budget of one slice did not give one workgroup for the generic class");
            Tt.capped_plans++;
        }
        std::vector<int32_t> dist(P.n_dist, INT32_MAX);
        std::vector<u64> best(P.n_best, 0), none;
        mine_host_run(P, C.qbytes.data(), C.qoff.data(), C.nq(), true, &dist, nullptr, &Tt.H);
        mine_host_run(P, C.qbytes.data(), C.qoff.data(), C.nq(), false, nullptr, &best, nullptr);
        Tt.plans++;
        uint64_t dist_off = 0, best_off = 0;
        for (const smx_mine_job &J : C.jobs) {
            std::vector<double> want_best(J.nt, 0.0);
            for (uint32_t qi = 0; qi < J.nq; qi++)
                for (uint32_t ti = 0; ti < J.nt; ti++) {
                    const uint32_t q = J.q0 + qi, t = J.t0 + ti;
                    const int m = (int)(C.qoff[q + 1] - C.qoff[q]), n = (int)(C.toff[t + 1] - C.toff[t]);
                    const int got = dist[dist_off + (uint64_t)qi * J.nt + ti];
                    int want = got;
                    if (ref) {
                        const int d = ref->at({q, t});
                        want = (n > 0 && k[q] >= 0 && d > k[q]) ? -1 : d;
                        Tt.compared++;
                        if (got != want) {
                            if (Tt.mismatches++ < 10) fprintf(stderr, "MISMATCH distance q=%u (m=%d k=%d) t=%u (n=%d): want %d, got %d\n", q, m, k[q], t, n, want, got);
                        }
                        (want >= 0 ? Tt.within : Tt.beyond)++;
                    } else if (got == INT32_MAX) {
                        host_twin_fail("a distance was not written");
                    }
                    if (want != -1) {
                        const double identity = 1.0 - (double)want / (double)m;
                        if (identity >= J.min_identity && identity > 0.0 && identity > want_best[ti]) want_best[ti] = identity;
                    }
                }
            for (uint32_t ti = 0; ti < J.nt; ti++) {
                u64 bits;
                memcpy(&bits, &want_best[ti], 8);
                Tt.compared++;
                Tt.best_set += bits != 0;
                if (best[best_off + ti] != bits) {
                    if (Tt.mismatches++ < 10) fprintf(stderr, "MISMATCH best identity job t0=%u ti=%u: want %.17g\n", J.t0, ti, want_best[ti]);
                }
            }
            dist_off += (uint64_t)J.nq * J.nt;
            best_off += J.nt;
        }
        if (dist_off != P.n_dist || best_off != P.n_best) host_twin_fail("the plan's output counts are not the jobs'");
    }
}

inline void mine_case_print(const MineCaseTotals &T) {
    long long searches = 0;
    const int sweep_rounds = chunk_owner_sweep(&searches);     // the owner search alone, up to four rounds
    printf("owner_sweep_rounds %d\nowner_sweep_searches %lld\n", sweep_rounds, searches);
    printf("plans %lld\ncapped_plans %lld\npairs %lld\nchunks %lld\nbuilds %lld\nblocks %lld\nrecords %lld\nrecords_two_chunks %lld\n"
           "blocks_inside %lld\nowner_rounds_max %lld\ncompared %lld\nwithin %lld\nbeyond %lld\nbest_set %lld\n",
           T.plans, T.capped_plans, T.H.pairs, T.H.chunks, T.H.builds, T.H.blocks, T.H.records, T.H.records_two_chunks,
           T.H.blocks_inside, T.H.owner_rounds_max, T.compared, T.within, T.beyond, T.best_set);
    for (int c = 0; c < 6; c++) printf("class_pairs_%d %lld\nclass_blocks_%d %lld\n", c, T.H.class_pairs[c], c, T.H.class_blocks[c]);
    printf("%lld mismatches\n", T.mismatches);
}

}  // namespace smx

#endif  // SMX_TESTS_MINE_CASES_H
