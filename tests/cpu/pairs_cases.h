// The clusters shapes of the plan tests, shared by the CPU simulation (tests/cpu/pairs_plan_sim.cpp, which checks every
// output element against a full-matrix NW DP) and the sanitizer driver (tests/asan/pairs_driver.cpp): jobs of 0 to 257
// reads, out of order and with gaps between them, reads of every state class and empty ones.
#ifndef SMX_TESTS_PAIRS_CASES_H
#define SMX_TESTS_PAIRS_CASES_H
#include <cstdio>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "pairs_host.h"

namespace smx {

struct PairsCase {
    std::string bytes;
    std::vector<uint64_t> off{0};
    std::vector<smx_pairs_job> jobs;
    uint32_t n_reads() const { return (uint32_t)off.size() - 1; }
    std::string read(uint32_t r) const { return bytes.substr(off[r], off[r + 1] - off[r]); }
    void add(const std::string &s) { bytes += s; off.push_back(bytes.size()); }
};

static const uint32_t kPairsJobSizes[10] = {33, 0, 257, 1, 128, 2, 31, 129, 32, 127};

// Most reads are light mutations of a few short centroids (class 1); every seventh is a mutated copy of a long centroid of
// one of the other classes (65, 130, 260, 520, 1030 bases: classes 2, 3, 4, 5 and 0) or empty.
inline PairsCase pairs_case(uint32_t seed) {
    std::mt19937 rng(seed);
    auto rand_seq = [&](int n) { std::string s(n, 'A'); for (char &c : s) c = "ACGT"[rng() % 4]; return s; };
    auto mutate = [&](const std::string &s, int per_mille) {
        std::string o;
        for (char c : s) {
            const int r = (int)(rng() % 1000);
            if (r < per_mille) o.push_back("ACGT"[rng() % 4]);
            else if (r < 2 * per_mille) { o.push_back(c); o.push_back("ACGT"[rng() % 4]); }
            else if (r >= 3 * per_mille) o.push_back(c);
        }
        return o;
    };
    std::vector<std::string> small, large;
    for (int m : {24, 40, 63}) small.push_back(rand_seq(m));
    for (int m : {65, 130, 260, 520, 1030}) large.push_back(rand_seq(m));
    PairsCase C;
    uint32_t x = 0;
    // the jobs in kPairsJobSizes order lie in the read array back to front, a stray read between two jobs
    std::vector<std::vector<std::string>> members;
    for (uint32_t n : kPairsJobSizes) {
        std::vector<std::string> mem;
        for (uint32_t i = 0; i < n; i++, x++) {
            if (x % 7 == 3) mem.push_back(x % 42 == 3 ? std::string() : mutate(large[(x / 7) % 5], 10 + (int)(rng() % 30)));
            else mem.push_back(mutate(small[x % 3], 20 + (int)(rng() % 60)));
        }
        members.push_back(mem);
    }
    C.jobs.resize(members.size());
    for (size_t j = members.size(); j-- > 0;) {
        C.jobs[j] = smx_pairs_job{C.n_reads(), (uint32_t)members[j].size()};
        for (const std::string &s : members[j]) C.add(s);
        C.add(rand_seq(30));                        // no job's read
    }
    return C;
}

// the limit per read: variant 0 none anywhere; variant 1 mixed (none, 0, a tenth of the length + 2, the length)
inline std::vector<int32_t> pairs_case_k(const PairsCase &C, int variant) {
    std::vector<int32_t> k(C.n_reads(), -1);
    if (variant)
        for (uint32_t r = 0; r < C.n_reads(); r++) {
            const int m = (int)(C.off[r + 1] - C.off[r]);
            const int kinds[5] = {m / 10 + 2, -1, m / 10 + 2, 0, m};
            k[r] = kinds[r % 5];
        }
    return k;
}

// NW distance by the O(nm) recurrence
inline int pairs_ref_nw(const std::string &a, const std::string &b) {
    const int m = (int)a.size(), n = (int)b.size();
    std::vector<int> col(m + 1);
    for (int i = 0; i <= m; i++) col[i] = i;
    for (int j = 1; j <= n; j++) {
        int diag = col[0];
        col[0] = j;
        for (int i = 1; i <= m; i++) {
            const int up = col[i - 1] + 1, left = col[i] + 1, sub = diag + (a[i - 1] == b[j - 1] ? 0 : 1);
            diag = col[i];
            col[i] = std::min(std::min(up, left), sub);
        }
    }
    return col[m];
}

struct PairsCaseTotals {
    PairsHostCounts H, HA;      // the distances runs, the neighbours runs
    long long plans = 0, capped_plans = 0, compared = 0, mismatches = 0, within = 0, beyond = 0, neighbours = 0;
};

// Plans and runs the case in both modes for the two limit variants under `budget_kind` (0: the production figure, 1: one
// slice of the generic class).  ref: NW distance of reads (a, b), a < b, or null: then the adjacency is checked against
// the twin's own distances alone.
inline void pairs_case_run(const PairsCase &C, int budget_kind, const std::map<std::pair<uint32_t, uint32_t>, int> *ref,
                           PairsCaseTotals *totals) {
    PairsCaseTotals &Tt = *totals;
    for (int variant = 0; variant < 2; variant++) {
        const std::vector<int32_t> k = pairs_case_k(C, variant);
        PairsPlan P, A;
        std::string why;
        const uint64_t budget = budget_kind == 1 ? chunk_slice_words(17) * 8 : CHUNK_SCRATCH_BYTES;   // 1030 bases and a few more
        const uint32_t n_jobs = (uint32_t)C.jobs.size();
        if (pairs_plan(true, C.bytes.data(), C.off.data(), C.n_reads(), C.jobs.data(), n_jobs, budget, &P, &why) != SMX_OK ||
            pairs_plan(false, C.bytes.data(), C.off.data(), C.n_reads(), C.jobs.data(), n_jobs, budget, &A, &why) != SMX_OK)
            host_twin_fail(why.c_str());
        if (budget_kind == 1) {
            if (P.words_max0 > 17) host_twin_fail("a read of the case is longer than the one-slice budget assumes");
            if (P.grid[0] != 1 || P.per_block[0] != P.chunks[0]) host_twin_fail("a budget of one slice did not give one workgroup for the generic class");
            Tt.capped_plans++;
        }
        std::vector<uint32_t> dist(P.n_out, 0x7fffffffu), adj(A.n_out, 0);
        pairs_host_run(P, k.data(), C.n_reads(), &dist, &Tt.H);
        pairs_host_run(A, k.data(), C.n_reads(), &adj, &Tt.HA);
        pairs_mirror(A, adj.data());
        Tt.plans++;
        uint64_t d_off = 0, a_off = 0;
        for (uint32_t jj = 0; jj < n_jobs; jj++) {
            const smx_pairs_job &J = C.jobs[jj];
            const uint32_t n = J.n, nw = (n + 31) / 32;
            if (P.jobs[jj].out_off != d_off || A.jobs[jj].out_off != a_off) host_twin_fail("a job's output offset is not the sum of the earlier jobs'");
            std::vector<uint32_t> want_adj((size_t)n * nw, 0);
            uint64_t at = d_off;
            for (uint32_t i = 0; i < n; i++)
                for (uint32_t j = i + 1; j < n; j++, at++) {
                    const uint32_t a = J.r0 + i, b = J.r0 + j;
                    const int got = (int)dist[at];
                    int want = got;
                    if (ref) {
                        const int d = ref->at({a, b});
                        const int lim = (k[a] < 0 || k[b] < 0) ? -1 : std::max(k[a], k[b]);
                        want = (lim >= 0 && d > lim) ? -1 : d;
                        Tt.compared++;
                        if (got != want && Tt.mismatches++ < 10)
                            fprintf(stderr, "MISMATCH distance job %u (n=%u) i=%u j=%u k=%d: want %d, got %d\n", jj, n, i, j, lim, want, got);
                        (want >= 0 ? Tt.within : Tt.beyond)++;
                    } else if (got == 0x7fffffff) {
                        host_twin_fail("a distance was not written");
                    }
                    if (want >= 0) {
                        want_adj[(size_t)i * nw + j / 32] |= 1u << (j % 32);
                        want_adj[(size_t)j * nw + i / 32] |= 1u << (i % 32);
                        Tt.neighbours++;
                    }
                }
            // the whole matrix: symmetric, zero diagonal and zero bits at positions >= n by construction of want_adj
            for (size_t w = 0; w < want_adj.size(); w++) {
                Tt.compared++;
                if (adj[a_off + w] != want_adj[w] && Tt.mismatches++ < 10)
                    fprintf(stderr, "MISMATCH adjacency job %u (n=%u) row %zu word %zu: want %08x, got %08x\n", jj, n, w / nw, w % nw, want_adj[w], adj[a_off + w]);
            }
            d_off += (uint64_t)n * (n ? n - 1 : 0) / 2;
            a_off += (uint64_t)n * nw;
        }
        if (d_off != P.n_out || a_off != A.n_out) host_twin_fail("the plan's output counts are not the jobs'");
    }
}

inline void pairs_case_print(const PairsCaseTotals &T) {
    printf("plans %lld\ncapped_plans %lld\npairs %lld\nchunks %lld\nbuilds %lld\nblocks %lld\nrows %lld\nrows_late %lld\nword_stores %lld\n"
           "words_guarded %lld\nblocks_inside %lld\nowner_rounds_max %lld\ncompared %lld\nwithin %lld\nbeyond %lld\nneighbours %lld\n",
           T.plans, T.capped_plans, T.H.pairs, T.H.chunks, T.H.builds, T.H.blocks, T.H.records, T.H.rows_late, T.HA.word_stores,
           T.HA.words_guarded, T.H.blocks_inside, T.H.owner_rounds_max, T.compared, T.within, T.beyond, T.neighbours);
    for (int c = 0; c < 6; c++) printf("class_pairs_%d %lld\n", c, T.H.class_pairs[c]);
    printf("%lld mismatches\n", T.mismatches);
}

}  // namespace smx

#endif  // SMX_TESTS_PAIRS_CASES_H
