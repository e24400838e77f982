// CPU simulation of the tree call (specimux_amd/csrc/smx_nj.hip): the host plan (smx_nj_plan.h) and the kernels as host
// loops (nj_host.h over smx_nj_core.h), with the reductions and the threads of a phase visited forwards, reversed and
// shuffled, against a plain triple loop of the algorithm as DESIGN.md §22 states it.  Built by tests/test_nj_cpu.py with
// g++ -ffp-contract=off; prints counters and "<n> mismatches".  usage: nj_sim <seed>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "nj_host.h"

using namespace smx;

static uint64_t mismatches = 0;
static void expect(bool ok, const char *what, uint32_t n, const char *kind) {
    if (!ok) {
        mismatches++;
        printf("MISMATCH %s n=%u %s\n", what, n, kind);
    }
}

// The algorithm, plainly: a full matrix, pairs scanned in the order (lo, hi) with a strict <.
static void nj_plain(const std::vector<int32_t> &tri, uint32_t n, NjHostResult *out) {
    std::vector<std::vector<double>> d(n, std::vector<double>(n, 0.0));
    std::vector<double> r(n);
    std::vector<uint32_t> node(n);
    for (uint32_t i = 0; i < n; i++) {
        long long s = 0;
        for (uint32_t j = 0; j < n; j++) {
            if (i == j) continue;
            const int32_t v = tri[i < j ? nj_tri_index(i, j, n) : nj_tri_index(j, i, n)];
            d[i][j] = (double)v;
            s += v;
        }
        r[i] = (double)s;
        node[i] = i;
    }
    out->merges.clear();
    uint32_t na = n;
    for (uint32_t t = 0; na > 3; t++) {
        const double c = (double)(na - 2);
        double best = 0.0;
        uint32_t lo = 0, hi = 0;
        bool any = false;
        for (uint32_t i = 0; i < na; i++)
            for (uint32_t j = i + 1; j < na; j++) {
                const double q = nj_q(c, d[i][j], r[i], r[j]);
                if (!any || q < best) { any = true; best = q; lo = i; hi = j; }
            }
        const double dl = d[lo][hi], ra = r[lo], rb = r[hi];
        smx_nj_merge m;
        memset(&m, 0, sizeof m);
        m.a = node[lo]; m.b = node[hi]; m.n_active = na; m.d = dl; m.ra = ra; m.rb = rb;
        out->merges.push_back(m);
        for (uint32_t k = 0; k < na; k++) {
            if (k == lo || k == hi) continue;
            const double duk = nj_duk(d[lo][k], d[hi][k], dl);
            r[k] = nj_r_other(r[k], d[lo][k], d[hi][k], duk);
            d[lo][k] = d[k][lo] = duk;
        }
        r[lo] = nj_r_new(ra, rb, (double)na, dl);
        node[lo] = n + t;
        const uint32_t last = na - 1;
        if (hi != last) {
            for (uint32_t k = 0; k < na; k++) d[hi][k] = d[last][k];
            for (uint32_t k = 0; k < na; k++) d[k][hi] = d[k][last];
            r[hi] = r[last];
            node[hi] = node[last];
        }
        d[hi][hi] = 0.0;
        na--;
    }
    for (uint32_t i = 0; i < 3; i++) out->last[i] = i < n ? node[i] : 0u;
    out->last_d[0] = n >= 2 ? d[0][1] : 0.0;
    out->last_d[1] = n >= 3 ? d[0][2] : 0.0;
    out->last_d[2] = n >= 3 ? d[1][2] : 0.0;
}

static bool same(const NjHostResult &a, const NjHostResult &b) {
    return a.merges.size() == b.merges.size() &&
           (a.merges.empty() || memcmp(a.merges.data(), b.merges.data(), a.merges.size() * sizeof(smx_nj_merge)) == 0) &&
           memcmp(a.last, b.last, sizeof a.last) == 0 && memcmp(a.last_d, b.last_d, sizeof a.last_d) == 0;
}

static std::vector<int32_t> make(const char *kind, uint32_t n, std::mt19937 &rng) {
    std::vector<int32_t> tri((size_t)n * (n ? n - 1 : 0) / 2);
    const std::string k(kind);
    size_t at = 0;
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t j = i + 1; j < n; j++, at++) {
            if (k == "random") tri[at] = 1 + (int32_t)(rng() % 3000);
            else if (k == "narrow") tri[at] = 1 + (int32_t)(rng() % 3);       // many equal Q
            else if (k == "equal") tri[at] = 7;
            else if (k == "zero") tri[at] = 0;
            else if (k == "ladder") tri[at] = 3 * (int32_t)j + 1 + (int32_t)((i + j) % 2);
            else if (k == "largest") tri[at] = INT32_MAX;
        }
    return tri;
}

int main(int argc, char **argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 10) : 1u;
    std::mt19937 rng(seed);
    NjCounters K;
    uint64_t cases = 0, merges_checked = 0;
    std::vector<uint32_t> sizes = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 100, 255, 256, 257};
    if (seed == 1) sizes.push_back(1030);        // more than one slot per join thread, once: the cost grows with n^3
    for (uint32_t n : sizes)
        for (const char *kind : {"random", "narrow", "equal", "zero", "ladder", "largest"}) {
            const std::string k(kind);
            if (n > 260 && k != "random") continue;
            if (k == "largest" && n > 64) continue;
            const std::vector<int32_t> tri = make(kind, n, rng);
            NjHostResult want;
            nj_plain(tri, n, &want);
            for (NjOrder order : {NJ_FORWARD, NJ_REVERSED, NJ_SHUFFLED}) {
                NjHostResult got;
                std::string why;
                const int rc = nj_host_call(tri.data(), n, order, seed * 7919u + n, &got, &K, &why);
                expect(rc == SMX_OK, "status", n, kind);
                expect(same(got, want), "records", n, kind);
            }
            if (k == "largest" && n == 64) {      // the row sums are exact: 63 (2^31 - 1), far above 2^32
                expect(!want.merges.empty() && want.merges[0].ra == 63.0 * 2147483647.0, "row sum", n, kind);
            }
            cases++;
            merges_checked += 3 * want.merges.size();
        }
    // the plan: sizes, launch counts, refusals, and the answers of n <= 3
    uint64_t refusals = 0;
    {
        NjPlan P;
        std::string why;
        smx_nj_merge m = {};
        uint32_t last[3] = {0, 0, 0};
        double last_d[3] = {0, 0, 0};
        std::vector<int32_t> tri = make("random", 10, rng);
        expect(nj_plan(tri.data(), 10, &m, last, last_d, &P, &why) == SMX_OK && P.iterations == 7 && P.launches == 15 &&
               P.tri_entries == 45 && P.d_bytes == 800 && P.r_bytes == 80 && P.node_bytes == 40 && P.merges_bytes == 7 * 40 &&
               P.init_grid == 10 && P.rowmin_grid_max == 3, "plan of 10", 10, "plan");
        expect(nj_plan(nullptr, 10, &m, last, last_d, &P, &why) == SMX_ERR_ARG, "null tri", 10, "plan"); refusals++;
        expect(nj_plan(tri.data(), 10, nullptr, last, last_d, &P, &why) == SMX_ERR_ARG, "null merges", 10, "plan"); refusals++;
        expect(nj_plan(tri.data(), 10, &m, nullptr, last_d, &P, &why) == SMX_ERR_ARG, "null last", 10, "plan"); refusals++;
        expect(nj_plan(tri.data(), 10, &m, last, nullptr, &P, &why) == SMX_ERR_ARG, "null last_d", 10, "plan"); refusals++;
        expect(nj_plan(tri.data(), SMX_NJ_MAX_N + 1, &m, last, last_d, &P, &why) == SMX_ERR_UNSUPPORTED, "too large", 0, "plan"); refusals++;
        tri[44] = -1;
        expect(nj_plan(tri.data(), 10, &m, last, last_d, &P, &why) == SMX_ERR_ARG && why.find("44") != std::string::npos,
               "negative entry", 10, "plan"); refusals++;
        expect(nj_plan(tri.data(), 9, &m, last, last_d, &P, &why) == SMX_OK, "the entry behind the triangle is not read", 9, "plan");
        // n <= 3: no tri needed below 2, no merges needed at all
        expect(nj_plan(nullptr, 1, nullptr, last, last_d, &P, &why) == SMX_OK && P.launches == 0, "n = 1", 1, "plan");
        expect(nj_plan(nullptr, 2, nullptr, last, last_d, &P, &why) == SMX_ERR_ARG, "n = 2 without tri", 2, "plan"); refusals++;
        const int32_t three[3] = {5, 6, 9};
        nj_small(three, 0, last, last_d);
        expect(last[0] == 0 && last[1] == 0 && last[2] == 0 && last_d[0] == 0 && last_d[1] == 0 && last_d[2] == 0, "small", 0, "plan");
        nj_small(three, 1, last, last_d);
        expect(last[0] == 0 && last[1] == 0 && last[2] == 0 && last_d[0] == 0 && last_d[1] == 0 && last_d[2] == 0, "small", 1, "plan");
        nj_small(three, 2, last, last_d);
        expect(last[0] == 0 && last[1] == 1 && last[2] == 0 && last_d[0] == 5 && last_d[1] == 0 && last_d[2] == 0, "small", 2, "plan");
        nj_small(three, 3, last, last_d);
        expect(last[0] == 0 && last[1] == 1 && last[2] == 2 && last_d[0] == 5 && last_d[1] == 6 && last_d[2] == 9, "small", 3, "plan");
        expect(nj_rowmin_grid(4) == 1 && nj_rowmin_grid(5) == 1 && nj_rowmin_grid(6) == 2, "rowmin grid", 0, "plan");
    }
    printf("cases %llu\nmerges_checked %llu\niterations %llu\nties %llu\nmoves_none %llu\nmoves %llu\nrowmin_rows %llu\n"
           "rowmin_entries %llu\njoin_slots %llu\nrefusals_checked %llu\n",
           (unsigned long long)cases, (unsigned long long)merges_checked, (unsigned long long)K.iterations,
           (unsigned long long)K.ties, (unsigned long long)K.moves_none, (unsigned long long)K.moves,
           (unsigned long long)K.rowmin_rows, (unsigned long long)K.rowmin_entries, (unsigned long long)K.join_slots,
           (unsigned long long)refusals);
    printf("%llu mismatches\n", (unsigned long long)mismatches);
    return mismatches ? 1 : 0;
}
