// CPU twin of the alignment kernels behind smx_align and smx_align_batch (specimux_amd/csrc/smx_align.hip): their lane
// bodies (smx_align_lane.h, the same source lines, compiled for the host by tests/cpu/align_host.h) against a plain
// full-matrix DP written from oracle/edlib_semantics.py's align_py -- HW and SHW, the 28 IUPAC pairs with code 15 never
// matching, the start rule "smallest start whose NW distance equals best".  Every buffer has exactly the size
// smx_calls.cpp allocates.  Built and run by tests/test_align_cpu.py (g++, no GPU).
//
//   align_sim exhaustive      every query of 1..4 and target of 1..7 letters over {A, C, N, x}, both modes, k = 0..5 (so
//                             k >= m is in), cap in {0, 1, nloc}
//   align_sim wrap            the byte-wide score column: queries of 1..64 letters, targets of up to 2000 letters that
//                             start with the query, hold no matching letter or are random over two letters, k up to 1000
//   align_sim random <seed>   launches of 1..400 alignments: targets of 1..400 letters with lower-case and other bytes,
//                             copies planted at column 0 and at the last column, k up to 250, every cap
//   align_sim cases           some hundred cases of the three sets with the reference's answer, for the oracle:
//                             "CASE <query> <target in hex> <mode> <k> <dist> <start:end,...|->"
//
// Prints "<counter> <value>" lines (the Python test asserts lower bounds on them) and "<n> mismatches".
#include <cstdlib>

#include "align_host.h"

using namespace align_host;

static Stats S;

static const char *kQueryAlphabet = "ACGTACGTACGTACGTACGTACGTNRYKMSWBDHV";
static const char *kTargetAlphabet = "ACGTACGTACGTACGTACGTACGTACGTACGTNRYKMSWBDHVaxacgtn?-\xff";
static const int kRandomM[10] = {1, 5, 13, 20, 23, 31, 32, 33, 47, 64};
static const int kRandomN[12] = {1, 64, 65, 129, 400, 2, 63, 200, 400, 300, 17, 128};

struct RandomCase {
    unsigned qi;
    std::string t;
    int k, mode;
};
// One launch of the random set.  Alignment `it` of a launch: it % 4 plants a copy of the query (0: mutated, anywhere;
// 1: at column 0; 2: ending at the last column; 3: none), it % 8 picks k (0, 1, 3, 7, m - 1, m, m + 1..250, 250) and
// (it / 8) % 2 the mode, so that every launch of 16 or more lanes holds every plant with k < m and k >= m in both modes.
// The counters the Python test bounds from below follow from these rules and the launch sizes alone.
static void random_launch(std::mt19937_64 &rng, int n, std::vector<std::string> *queries, std::vector<RandomCase> *cases) {
    auto uni = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    auto pick = [&](const char *alphabet) { return alphabet[rng() % strlen(alphabet)]; };
    const int nq = uni(1, 11);
    for (int x = 0; x < nq; x++) {
        std::string q(kRandomM[rng() % 10], 'A');
        for (char &c : q) c = pick(kQueryAlphabet);
        if (x == 1) q = "N";
        queries->push_back(q);
    }
    for (int it = 0; it < n; it++) {
        RandomCase c;
        c.qi = (unsigned)(rng() % queries->size());
        const std::string &q = (*queries)[c.qi];
        const int m = (int)q.size();
        int nt = rng() % 8 == 0 ? uni(151, 400) : uni(1, 150);
        if (it % 4 == 1 || it % 4 == 2) nt = std::max(nt, m);
        if (it % 16 == 8) nt = std::max(nt, m + 1);   // SHW, k = 0: the scan stops short of the target's end
        // no letter of the target matches: HW with k = 250 (it % 32 == 7) has every one of at least 17 columns optimal,
        // HW with k = 0 (it % 32 == 16) is above k
        const bool barren = it % 32 == 7 || it % 32 == 16;
        if (barren) nt = std::max(nt, 17);
        c.t.assign(nt, 'A');
        for (char &ch : c.t) ch = barren ? pick("xa?-") : pick(kTargetAlphabet);
        if (barren) S.count["no_matching_letter"]++;
        std::string copy = q;
        if (barren) {
        } else if (it % 4 == 0 && nt > m) {
            for (int e = uni(0, 4); e > 0; e--) copy[rng() % m] = "ACGT"[rng() % 4];
            c.t.replace(uni(0, nt - m), m, copy);
        } else if (it % 4 == 1) {
            c.t.replace(0, m, copy);
            S.count["planted_at_0"]++;
        } else if (it % 4 == 2) {
            c.t.replace(nt - m, m, copy);
            S.count["planted_at_end"]++;
        }
        const int ks[8] = {0, 1, 3, 7, m - 1, m, uni(m + 1, 250), 250};
        c.k = ks[it % 8];
        c.mode = (it / 8) % 2;
        cases->push_back(c);
    }
}

static void run_random(uint64_t seed) {
    std::mt19937_64 rng(seed * 0x9E3779B97F4A7C15ull + 7);
    OutPool pool;
    for (int n : kRandomN) {
        std::vector<std::string> qs;
        std::vector<RandomCase> cases;
        random_launch(rng, n, &qs, &cases);
        std::vector<Query> Q;
        for (const std::string &q : qs) Q.emplace_back(q);
        std::vector<const Query *> queries;
        for (const Query &q : Q) queries.push_back(&q);
        std::vector<Target> T;
        T.reserve(cases.size());
        std::vector<Ref> refs;
        refs.reserve(cases.size());
        std::vector<Item> items;
        int most = 0;
        for (const RandomCase &c : cases) {
            T.emplace_back(c.t);
            refs.push_back(ref_align(qs[c.qi], c.t, c.mode));
            const Ref &r = refs.back();
            const int m = (int)qs[c.qi].size(), nloc = r.best > c.k ? 0 : (int)r.ends.size();
            most = std::max(most, nloc);
            check_single(S, Q[c.qi], T.back(), c.mode, c.k, r, {0, 1, nloc}, pool);
            items.push_back(Item{c.qi, &T.back(), c.k, c.mode, &r});
            S.count["alignments"]++;
            if (c.k >= m) S.count[c.mode ? "k_ge_m_shw" : "k_ge_m_hw"]++;
            if (c.k == 250) S.count["k_250"]++;
            if (c.mode == 1 && (int)c.t.size() > m + std::min(c.k, m)) S.count["shw_trimmed"]++;
            if (nloc == 0) S.count["above_k"]++;
            if (nloc > 16) S.count["more_than_16_locations"]++;
            for (char ch : c.t)
                if (code_of((unsigned char)ch) == 15) { S.count["targets_with_other_bytes"]++; break; }
        }
        // every cap of the issue, over workspaces that hold what another call left
        const unsigned caps[5] = {0, 1, 16, (unsigned)std::max(most - 1, 0), (unsigned)most};
        for (int x = 0; x < 5; x++) check_batch(S, queries, items, caps[x], (unsigned char)(x * 0x3F));
        // the same request after a larger one: a workspace full of the larger call's scores (here: random bytes) changes
        // nothing, as both runs are held against the reference
        check_batch(S, queries, items, (unsigned)most, (unsigned char)rng() | 1);
        S.count["launches_repeated"]++;
        S.count["launches"]++;
        if (n % 64 == 1) S.count["launches_one_lane_in_last_wave"]++;
        if (n % 64 == 0) S.count["launches_full_last_wave"]++;
    }
}

static void print_case(const std::string &q, const std::string &t, int mode, int k) {
    const Ref r = ref_align(q, t, mode);
    printf("CASE %s ", q.c_str());
    for (unsigned char c : t) printf("%02x", c);
    printf(" %d %d %d ", mode, k, r.best > k ? -1 : r.best);
    if (r.best > k) printf("-");
    else
        for (size_t x = 0; x < r.ends.size(); x++) printf("%s%d:%d", x ? "," : "", r.starts[x], r.ends[x]);
    printf("\n");
    S.count["cases_printed"]++;
}

static void run_cases() {
    long long at = 0;
    wrap_cases([&](const std::string &q, const std::string &t, int k, bool) {
        if (at++ % 13 == 0) print_case(q, t, (int)(at % 2), k);
    });
    std::mt19937_64 rng(99);
    std::vector<std::string> qs;
    std::vector<RandomCase> cases;
    random_launch(rng, 200, &qs, &cases);
    for (const RandomCase &c : cases) print_case(qs[c.qi], c.t, c.mode, c.k);
    for (const char *key : {"planted_at_0", "planted_at_end", "no_matching_letter"}) S.count.erase(key);
    const char letters[4] = {'A', 'C', 'N', 'x'};
    for (int x = 0; x < 200; x++) {
        std::string q(1 + rng() % 4, 'A'), t(1 + rng() % 7, 'A');
        for (char &c : q) c = letters[rng() % 3];
        for (char &c : t) c = letters[rng() % 4];
        print_case(q, t, (int)(rng() % 2), (int)(rng() % 6));
    }
}

int main(int argc, char **argv) {
    check_alphabet(S);
    if (argc >= 2 && !strcmp(argv[1], "exhaustive")) run_exhaustive(S);
    else if (argc >= 2 && !strcmp(argv[1], "wrap")) run_wrap(S);
    else if (argc >= 3 && !strcmp(argv[1], "random")) run_random(strtoull(argv[2], nullptr, 10));
    else if (argc >= 2 && !strcmp(argv[1], "cases")) run_cases();
    else {
        fprintf(stderr, "usage: align_sim exhaustive | wrap | random <seed> | cases\n");
        return 2;
    }
    for (auto &kv : S.count) printf("%s %lld\n", kv.first.c_str(), kv.second);
    printf("%lld mismatches\n", S.mismatches);
    return 0;
}
