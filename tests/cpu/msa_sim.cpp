// CPU simulation of smx_msa (specimux_amd/csrc/smx_msa.hip): the host plan (smx_msa_plan.h) and the kernels as host loops
// (msa_host.h over smx_msa_core.h), waves, lanes and threads visited forwards, reversed and shuffled, against a plain
// triple loop written from the rules of DESIGN.md §23 with nothing shared but the header's constants.  Pairs of lengths 1,
// 15 / 16 / 17, 63 / 64 / 65, 1025 (one row above a round of bands), 300 x 3 and 3 x 300, identical sequences, repeats of
// one base; trees of 3 .. 12 tips, balanced, ladder and random, under three pairs of weights and under a budget that
// cuts every level into launches of one merge.  Then the plan alone: levels, sizes, cutting, every refusal.
// Prints counters and "<k> mismatches"; built and run by tests/test_msa_sim_cpu.py.
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "msa_host.h"

using namespace smx;

static unsigned long long mismatches = 0, cases = 0, refusals_checked = 0, plan_checks = 0;

static void expect(bool ok, const char *what) {
    if (!ok) {
        mismatches++;
        printf("MISMATCH %s\n", what);
    }
}

// ---- the plain reference
typedef std::array<uint64_t, 6> Col;
struct Node { std::vector<uint32_t> tips; std::vector<std::string> rows; std::vector<Col> prof; };

static uint32_t code_of_byte(unsigned char ch) { return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4; }

static void plain_msa(const std::vector<std::string> &seqs, const std::vector<smx_msa_merge> &merges, uint64_t X, uint64_t G,
                      MsaHostResult *out) {
    const uint32_t n = (uint32_t)seqs.size();
    std::vector<Node> nodes(n + merges.size());
    for (uint32_t i = 0; i < n; i++) {
        nodes[i].tips = {i};
        nodes[i].rows = {seqs[i]};
        for (unsigned char ch : seqs[i]) {
            Col c = {0, 0, 0, 0, 0, 0};
            c[code_of_byte(ch)] = 1;
            nodes[i].prof.push_back(c);
        }
    }
    out->lens.clear();
    out->costs.clear();
    for (size_t t = 0; t < merges.size(); t++) {
        const Node &A = nodes[merges[t].a], &B = nodes[merges[t].b];
        const uint64_t na = A.tips.size(), nb = B.tips.size();
        const size_t La = A.prof.size(), Lb = B.prof.size();
        std::vector<uint64_t> ga(La + 1), gb(Lb + 1);
        for (size_t i = 1; i <= La; i++) ga[i] = G * (na - A.prof[i - 1][5]) * nb;
        for (size_t j = 1; j <= Lb; j++) gb[j] = G * (nb - B.prof[j - 1][5]) * na;
        auto s = [&](size_t i, size_t j) {
            const Col &a = A.prof[i - 1], &b = B.prof[j - 1];
            const uint64_t ra = na - a[5], rb = nb - b[5];
            uint64_t same = 0;
            for (int k = 0; k < 5; k++) same += a[k] * b[k];
            return X * (ra * rb - same) + G * (a[5] * rb + ra * b[5]);
        };
        std::vector<uint64_t> D((La + 1) * (Lb + 1));
        auto at = [&](size_t i, size_t j) -> uint64_t & { return D[i * (Lb + 1) + j]; };
        for (size_t i = 1; i <= La; i++) at(i, 0) = at(i - 1, 0) + ga[i];
        for (size_t j = 1; j <= Lb; j++) at(0, j) = at(0, j - 1) + gb[j];
        for (size_t i = 1; i <= La; i++)
            for (size_t j = 1; j <= Lb; j++)
                at(i, j) = std::min(std::min(at(i - 1, j - 1) + s(i, j), at(i - 1, j) + ga[i]), at(i, j - 1) + gb[j]);
        std::vector<int> ops;
        size_t i = La, j = Lb;
        while (i > 0 || j > 0) {
            if (i > 0 && j > 0 && at(i, j) == at(i - 1, j - 1) + s(i, j)) { ops.push_back(0); i--; j--; }
            else if (j == 0 || (i > 0 && at(i, j) == at(i - 1, j) + ga[i])) { ops.push_back(1); i--; }
            else { ops.push_back(2); j--; }
        }
        std::reverse(ops.begin(), ops.end());
        Node N;
        N.tips = A.tips;
        N.tips.insert(N.tips.end(), B.tips.begin(), B.tips.end());
        N.rows.assign(na + nb, std::string());
        size_t ia = 0, ib = 0;
        for (int op : ops) {
            Col c = {0, 0, 0, 0, 0, 0};
            if (op != 2) for (int k = 0; k < 6; k++) c[k] += A.prof[ia][k];
            if (op != 1) for (int k = 0; k < 6; k++) c[k] += B.prof[ib][k];
            if (op == 1) c[5] += nb;
            if (op == 2) c[5] += na;
            N.prof.push_back(c);
            for (size_t r = 0; r < na; r++) N.rows[r].push_back(op != 2 ? A.rows[r][ia] : '-');
            for (size_t r = 0; r < nb; r++) N.rows[na + r].push_back(op != 1 ? B.rows[r][ib] : '-');
            if (op != 2) ia++;
            if (op != 1) ib++;
        }
        out->lens.push_back((uint32_t)ops.size());
        out->costs.push_back(at(La, Lb));
        nodes[n + t] = N;
    }
    const Node &root = nodes.back();
    out->n_cols = (uint32_t)root.prof.size();
    out->rows.assign((size_t)n * out->n_cols, 0);
    for (size_t r = 0; r < root.tips.size(); r++) memcpy(&out->rows[(size_t)root.tips[r] * out->n_cols], root.rows[r].data(), out->n_cols);
}

// ---- generators
static std::string random_seq(std::mt19937 &rng, size_t len, const char *alphabet = "ACGT") {
    std::string s(len, 'A');
    const size_t k = strlen(alphabet);
    for (char &c : s) c = alphabet[rng() % k];
    return s;
}

static std::string mutate(std::mt19937 &rng, const std::string &s, unsigned per_mille) {
    std::string out;
    for (char c : s) {
        const unsigned r = rng() % 1000u;
        if (r < per_mille / 3) continue;
        if (r < 2 * per_mille / 3) { out.push_back("ACGT"[rng() % 4]); continue; }
        out.push_back(c);
        if (r < per_mille) out.push_back("ACGT"[rng() % 4]);
    }
    return out.empty() ? s.substr(0, 1) : out;
}

static std::vector<smx_msa_merge> tree_of(std::mt19937 &rng, uint32_t n, int kind) {   // 0 balanced, 1 ladder, 2 random
    std::vector<smx_msa_merge> m;
    std::vector<uint32_t> live(n);
    std::iota(live.begin(), live.end(), 0u);
    if (kind == 1) {
        uint32_t top = 0;
        for (uint32_t i = 1; i < n; i++) { m.push_back({top, i}); top = n + (uint32_t)m.size() - 1; }
        return m;
    }
    while (live.size() > 1) {
        if (kind == 0) {
            std::vector<uint32_t> next;
            for (size_t k = 0; k < live.size(); k += 2)
                if (k + 1 < live.size()) { m.push_back({live[k], live[k + 1]}); next.push_back(n + (uint32_t)m.size() - 1); }
                else next.push_back(live[k]);
            live = next;
        } else {
            const size_t a = rng() % live.size();
            size_t b = rng() % (live.size() - 1);
            if (b >= a) b++;
            m.push_back({live[a], live[b]});
            const uint32_t x = live[a], y = live[b];
            live.erase(std::remove_if(live.begin(), live.end(), [&](uint32_t v) { return v == x || v == y; }), live.end());
            live.push_back(n + (uint32_t)m.size() - 1);
        }
    }
    return m;
}

static MsaCounters K;

static void check_case(const std::vector<std::string> &seqs, const std::vector<smx_msa_merge> &merges, uint32_t X, uint32_t G,
                       uint64_t budget, const char *what) {
    std::string blob;
    std::vector<uint64_t> off(1, 0);
    for (const std::string &s : seqs) { blob += s; off.push_back(blob.size()); }
    MsaHostResult want;
    plain_msa(seqs, merges, X, G, &want);
    for (MsaOrder order : {MSA_FORWARD, MSA_REVERSED, MSA_SHUFFLED}) {
        MsaHostResult got;
        std::string why;
        const int rc = msa_host_call(blob.data(), off.data(), (uint32_t)seqs.size(), merges.data(), X, G, SMX_MSA_MAX_COLS, budget,
                                     order, 99u + (uint32_t)cases, &got, &K, &why);
        expect(rc == SMX_OK, what);
        expect(got.n_cols == want.n_cols && got.lens == want.lens && got.costs == want.costs, what);
        expect(got.rows == want.rows, what);
    }
    cases++;
}

// `msa_sim time <n>`: the host loops alone, forwards, on n sequences of about 650 nt up to 15 % from one ancestor under a
// balanced tree -- the smallest shape of tools/msa_bench.py, for scale.  Prints the wall time.
static int time_host_loops(uint32_t n) {
    std::mt19937 rng(1);
    const std::string root = random_seq(rng, 650);
    std::string blob;
    std::vector<uint64_t> off(1, 0);
    for (uint32_t i = 0; i < n; i++) { blob += mutate(rng, root, rng() % 151u); off.push_back(blob.size()); }
    const std::vector<smx_msa_merge> merges = tree_of(rng, n, 0);
    MsaHostResult got;
    MsaCounters C;
    std::string why;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = msa_host_call(blob.data(), off.data(), n, merges.data(), 1, 1, SMX_MSA_MAX_COLS, MSA_DEFAULT_BUDGET, MSA_FORWARD, 1u,
                                 &got, &C, &why);
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("host_loops n %u columns %u cells %llu wall_s %.3f status %d\n", n, got.n_cols, (unsigned long long)C.cells, s, rc);
    return rc == SMX_OK ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc > 2 && !strcmp(argv[1], "time")) return time_host_loops((uint32_t)atoi(argv[2]));
    std::mt19937 rng(argc > 1 ? (unsigned)atoi(argv[1]) : 1u);
    const bool big = argc > 1 && atoi(argv[1]) == 1;
    // pairs
    const uint32_t sizes[] = {1, 2, 15, 16, 17, 63, 64, 65, 129};
    for (uint32_t la : sizes)
        for (uint32_t lb : sizes) {
            const std::string a = random_seq(rng, la);
            std::string b = la == lb ? mutate(rng, a, 150) : random_seq(rng, lb);
            check_case({a, b}, {{0, 1}}, 1, 1, MSA_DEFAULT_BUDGET, "pair");
            check_case({a, b}, {{1, 0}}, 2, 3, MSA_DEFAULT_BUDGET, "pair swapped");
        }
    check_case({random_seq(rng, 300), random_seq(rng, 3)}, {{0, 1}}, 1, 1, MSA_DEFAULT_BUDGET, "300 x 3");
    check_case({random_seq(rng, 3), random_seq(rng, 300)}, {{0, 1}}, 5, 2, MSA_DEFAULT_BUDGET, "3 x 300");
    check_case({random_seq(rng, 1), random_seq(rng, 300)}, {{0, 1}}, 1, 1, MSA_DEFAULT_BUDGET, "1 x 300");
    {
        const std::string a = random_seq(rng, 200);
        check_case({a, a}, {{0, 1}}, 1, 1, MSA_DEFAULT_BUDGET, "identical");
        std::string d = a;
        d.erase(80, 40);
        check_case({a, d}, {{0, 1}}, 1, 1, MSA_DEFAULT_BUDGET, "deletion");
        check_case({std::string(70, 'A'), std::string(45, 'A')}, {{0, 1}}, 1, 1, MSA_DEFAULT_BUDGET, "repeat");
        check_case({std::string(33, 'A'), std::string(90, 'A'), std::string(64, 'A')}, {{0, 1}, {3, 2}}, 2, 3, MSA_DEFAULT_BUDGET, "repeats");
        check_case({"ACGTNNacgtRYACGT", "ACGTNacgGTRACGT", "ACGNNacgtRYACG"}, {{1, 2}, {0, 3}}, 1, 1, MSA_DEFAULT_BUDGET, "other bytes");
    }
    if (big) {
        const std::string a = random_seq(rng, 1025);
        check_case({a, mutate(rng, a, 100)}, {{0, 1}}, 1, 1, MSA_DEFAULT_BUDGET, "1025");
        check_case({random_seq(rng, 1025), random_seq(rng, 1100)}, {{0, 1}}, 2, 3, MSA_DEFAULT_BUDGET, "1025 unrelated");
    }
    // trees
    for (uint32_t n = 3; n <= 12; n++)
        for (int kind = 0; kind < 3; kind++) {
            const std::string root = random_seq(rng, 30 + rng() % 60);
            std::vector<std::string> seqs;
            for (uint32_t i = 0; i < n; i++) seqs.push_back(mutate(rng, root, 100 + 20 * (i % 5)));
            const std::vector<smx_msa_merge> merges = tree_of(rng, n, kind);
            const uint32_t w[3][2] = {{1, 1}, {2, 3}, {5, 2}};
            check_case(seqs, merges, w[n % 3][0], w[n % 3][1], MSA_DEFAULT_BUDGET, "tree");
            check_case(seqs, merges, 1000, 1000, 1, "tree, one merge a launch");
        }
    // the plan: levels, the order of a level, cutting, sizes
    {
        const uint32_t n = 6;
        const smx_msa_merge merges[] = {{4, 5}, {0, 1}, {2, 3}, {7, 8}, {6, 9}};   // levels 1 1 1 2 3
        const uint64_t off[] = {0, 10, 30, 60, 100, 150, 210};
        std::string blob(210, 'A'), why;
        uint8_t rows = 0;
        uint32_t n_cols = 0, lens[5] = {0};
        uint64_t costs[5] = {0};
        MsaPlan P;
        expect(msa_plan(blob.data(), off, n, merges, 1, 1, &rows, &n_cols, lens, costs, &P, &why) == SMX_OK, "plan");
        expect(P.n_levels == 3 && P.order == std::vector<uint32_t>({0, 1, 2, 3, 4}) &&
               P.level_start == std::vector<uint32_t>({0, 3, 4, 5}), "levels");
        expect(P.tips[10] == 6 && P.tips[9] == 4 && P.parent[10] == MSA_NONE && P.parent[6] == 10 && P.parent[0] == 7, "tips and parents");
        MsaState S;
        msa_state_init(P, off, &S);
        expect(S.prof_used == 210 && S.prof_off[5] == 150 && S.len[3] == 40, "tip profiles");
        std::vector<MsaLaunch> L;
        msa_level_launches(P, merges, S, 1, MSA_DEFAULT_BUDGET, &L);
        expect(L.size() == 1 && L[0].first == 0 && L[0].count == 3, "one launch");
        // merge 0: 50 x 60 -> 50 * 4 words, 110 bytes, 61 scores; merge 1: 10 x 20 -> 10 * 2, 30, 21; merge 2: 30 x 40 -> 30 * 3, 70, 41
        expect(L[0].tb_words == 200 + 20 + 90 && L[0].ops_bytes == 110 + 30 + 70 && L[0].row_entries == 61 + 21 + 41, "scratch sizes");
        msa_level_launches(P, merges, S, 1, 800 + 110 + 488 + 80 + 30 + 168, &L);   // the first two fit exactly
        expect(L.size() == 2 && L[0].count == 2 && L[1].first == 2 && L[1].count == 1, "cut in two");
        msa_level_launches(P, merges, S, 1, 1, &L);
        expect(L.size() == 3 && L[2].first == 2 && L[2].count == 1, "one merge always goes");
        std::vector<MsaMergeDev> recs;
        msa_level_launches(P, merges, S, 1, MSA_DEFAULT_BUDGET, &L);
        msa_launch_records(P, merges, L[0], &S, &recs);
        expect(recs.size() == 3 && recs[0].t == 0 && recs[0].La == 50 && recs[0].Lb == 60 && recs[0].prof_out == 210 &&
               recs[1].prof_out == 320 && recs[1].tb == 200 && recs[1].ops == 110 && recs[1].row == 61 && recs[2].map_a == 140 &&
               recs[2].map_b == 170 && S.prof_used == 210 + 110 + 30 + 70 && S.map_used == 210, "records");
        uint32_t done[5] = {110, 30, SMX_MSA_MAX_COLS + 1, 0, 0};
        expect(msa_launch_done(P, L[0], done, &S, &why) == SMX_ERR_UNSUPPORTED && S.len[6] == 110 && S.len[7] == 30, "a node too long");
        plan_checks += 9;
        // refusals
        struct { int want; const char *word; } r;
        auto refuse = [&](int rc, int want, const char *word) {
            expect(rc == want && why.find(word) != std::string::npos, word);
            refusals_checked++;
        };
        (void)r;
        refuse(msa_plan(nullptr, off, n, merges, 1, 1, &rows, &n_cols, lens, costs, &P, &why), SMX_ERR_ARG, "null");
        refuse(msa_plan(blob.data(), nullptr, n, merges, 1, 1, &rows, &n_cols, lens, costs, &P, &why), SMX_ERR_ARG, "null");
        refuse(msa_plan(blob.data(), off, n, nullptr, 1, 1, &rows, &n_cols, lens, costs, &P, &why), SMX_ERR_ARG, "null");
        refuse(msa_plan(blob.data(), off, n, merges, 1, 1, nullptr, &n_cols, lens, costs, &P, &why), SMX_ERR_ARG, "null");
        refuse(msa_plan(blob.data(), off, n, merges, 1, 1, &rows, nullptr, lens, costs, &P, &why), SMX_ERR_ARG, "null");
        refuse(msa_plan(blob.data(), off, n, merges, 1, 1, &rows, &n_cols, nullptr, costs, &P, &why), SMX_ERR_ARG, "null");
        refuse(msa_plan(blob.data(), off, n, merges, 1, 1, &rows, &n_cols, lens, nullptr, &P, &why), SMX_ERR_ARG, "null");
        refuse(msa_plan(blob.data(), off, n, merges, 0, 1, &rows, &n_cols, lens, costs, &P, &why), SMX_ERR_ARG, "weights");
        refuse(msa_plan(blob.data(), off, n, merges, 1, 1001, &rows, &n_cols, lens, costs, &P, &why), SMX_ERR_ARG, "weights");
        refuse(msa_plan(blob.data(), off, SMX_MSA_MAX_N + 1, merges, 1, 1, &rows, &n_cols, lens, costs, &P, &why), SMX_ERR_UNSUPPORTED, "above");
        const uint64_t empty[] = {0, 10, 10, 60, 100, 150, 210}, longer[] = {0, 10, 30, 60, 100, 150, 150 + SMX_MSA_MAX_COLS + 1};
        refuse(msa_plan(blob.data(), empty, n, merges, 1, 1, &rows, &n_cols, lens, costs, &P, &why), SMX_ERR_ARG, "empty");
        refuse(msa_plan(blob.data(), longer, n, merges, 1, 1, &rows, &n_cols, lens, costs, &P, &why), SMX_ERR_UNSUPPORTED, "longer");
        const smx_msa_merge self[] = {{4, 4}, {0, 1}, {2, 3}, {7, 8}, {6, 9}}, young[] = {{4, 6}, {0, 1}, {2, 3}, {7, 8}, {6, 9}},
                            twice[] = {{4, 5}, {0, 1}, {2, 3}, {7, 8}, {6, 7}};
        refuse(msa_plan(blob.data(), off, n, self, 1, 1, &rows, &n_cols, lens, costs, &P, &why), SMX_ERR_ARG, "merge 0");
        refuse(msa_plan(blob.data(), off, n, young, 1, 1, &rows, &n_cols, lens, costs, &P, &why), SMX_ERR_ARG, "merge 0");
        refuse(msa_plan(blob.data(), off, n, twice, 1, 1, &rows, &n_cols, lens, costs, &P, &why), SMX_ERR_ARG, "merge 4");
        // n = 0 and n = 1 need no merges, lens or costs
        expect(msa_plan(nullptr, nullptr, 0, nullptr, 1, 1, nullptr, &n_cols, nullptr, nullptr, &P, &why) == SMX_OK && P.n_levels == 0, "n = 0");
        expect(msa_plan(blob.data(), off, 1, nullptr, 1, 1, &rows, &n_cols, nullptr, nullptr, &P, &why) == SMX_OK && P.n_nodes == 1, "n = 1");
        plan_checks += 2;
    }
    printf("cases %llu\nmerges %llu\ncells %llu\nticks %llu\ntiles %llu\nsteps %llu\nedge_ops %llu\nlaunches %llu\nwords %llu\n"
           "plan_checks %llu\nrefusals_checked %llu\n%llu mismatches\n", cases, (unsigned long long)K.merges,
           (unsigned long long)K.cells, (unsigned long long)K.ticks, (unsigned long long)K.tiles, (unsigned long long)K.steps,
           (unsigned long long)K.edge_ops, (unsigned long long)K.launches, (unsigned long long)K.words, plan_checks, refusals_checked,
           mismatches);
    return mismatches ? 1 : 0;
}
