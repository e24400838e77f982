// CPU simulation of the clusters kernel's per-pair code (specimux_amd/csrc/smx_pairs_core.h): the same host/device
// pairs_pair the gfx950 kernel runs, over a Peq table and byte -> row map built the way mine_build_peq builds them in
// LDS, checked against a plain O(mn) DP with edlib's NW semantics.  Every pair runs twice: through the register class
// the host driver would pick for the query's length, and through the generic class (pairs_pair<0>, state in a reused
// scratch slice).  Built and run by tests/test_pairs_cpu.py (g++, no GPU).
//
//   pairs_sim exhaustive         every {A, C} query of length 1-6 x every {A, C} target of length 0-7 x
//                                k = -1..max(m, n) + 1
//   pairs_sim random <seed>      structured random cases (see run_random), writes oracle_sample.txt in the cwd
//
// Prints "<counter> <value>" lines (the Python test asserts lower bounds on them) and "<n> mismatches".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "chunk_walk_host.h"   // chunk_with_wr; smx_chunk_plan.h: chunk_class, the state class a call gives a read
#include "smx_pairs_core.h"

using namespace smx;
typedef std::string Seq;   // bytes, any value 0x00-0xFF

// NW: D[m][n] with D[i][0] = i, D[0][j] = j
static int dp_unlimited(const Seq &q, const Seq &t) {
    const int m = (int)q.size(), n = (int)t.size();
    std::vector<int> col(m + 1);
    for (int i = 0; i <= m; i++) col[i] = i;
    for (int j = 0; j < n; j++) {
        int diag = col[0];
        col[0] = j + 1;
        const unsigned char c = (unsigned char)t[j];
        for (int i = 1; i <= m; i++) {
            const int up = col[i - 1] + 1, left = col[i] + 1, sub = diag + ((unsigned char)q[i - 1] == c ? 0 : 1);
            diag = col[i];
            col[i] = std::min(std::min(up, left), sub);
        }
    }
    return col[m];
}

static int limited(int d, int k) { return (k >= 0 && d > k) ? -1 : d; }

// The query as the kernel sees it in LDS: rows 1..nrows for its distinct bytes in byte order, row 0 all zero.
struct Query {
    int m, W, Wp;
    unsigned short rowmap[256];
    std::vector<u64> peq;
    explicit Query(const Seq &q) {
        m = (int)q.size();
        W = (m + 63) >> 6;
        Wp = W | 1;
        bool present[256] = {false};
        for (unsigned char c : q) present[c] = true;
        int base = 1;
        for (int c = 0; c < 256; c++) rowmap[c] = present[c] ? (unsigned short)base++ : (unsigned short)0;
        peq.assign((size_t)base * Wp, 0ull);
        for (int i = 0; i < m; i++) peq[(size_t)rowmap[(unsigned char)q[i]] * Wp + (i >> 6)] |= 1ull << (i & 63);
    }
};

// the register class the call picks (smx_chunk_plan.h): words of per-lane state, 0 = generic (global scratch)
static int reg_class(int W) { return CHUNK_CLASS_WORDS[chunk_class((size_t)W)]; }

struct Sim {
    std::mt19937_64 rng;
    // generic-class scratch, as a workgroup's slice: [word][lane], reused (never cleared) from pair to pair
    std::vector<u64> sP, sM;
    std::vector<int> sS;
    std::vector<mine_u4> tbuf;
    long long pairs = 0, calls = 0, mismatches = 0;
    std::map<std::string, long long> count;

    explicit Sim(uint64_t seed) : rng(seed) {}

    int run_pair(int wr, const Query &Q, const unsigned char *t, int n, int k) {
        return chunk_with_wr(wr, [&](auto WR) {
            if constexpr (WR > 0) {
                RegState<WR> st;
                return pairs_pair<WR>(st, Q.peq.data(), Q.rowmap, Q.m, Q.W, Q.Wp, k, t, n);
            } else {
                const size_t need = (size_t)std::max(Q.W, 1) * MINE_THREADS;
                if (sP.size() < need) {   // grow with junk: the kernel's scratch is never initialised either
                    const size_t old = sP.size();
                    sP.resize(need); sM.resize(need); sS.resize(need);
                    for (size_t i = old; i < need; i++) { sP[i] = rng(); sM[i] = rng(); sS[i] = (int)(rng() >> 40); }
                }
                const int lane = (int)(rng() % MINE_THREADS);
                GlobalState st{sP.data() + lane, sM.data() + lane, sS.data() + lane};
                return pairs_pair<0>(st, Q.peq.data(), Q.rowmap, Q.m, Q.W, Q.Wp, k, t, n);
            }
        });
    }

    // one (query, target) with every k of ks against the unlimited DP distance d
    void check(const Query &Q, const Seq &t, int d, const std::vector<int> &ks, const char *kind) {
        const int n = (int)t.size();
        // the target as the host driver uploads it: 16-byte aligned; the slack past n holds junk here
        tbuf.assign((size_t)n / 16 + 1, mine_u4{0, 0, 0, 0});
        unsigned char *tb = reinterpret_cast<unsigned char *>(tbuf.data());
        for (size_t i = n; i < tbuf.size() * 16; i++) tb[i] = (unsigned char)rng();
        memcpy(tb, t.data(), (size_t)n);
        pairs++;
        count[std::string("kind_") + kind]++;
        const int wr = reg_class(Q.W);
        count["class_" + std::to_string(wr)]++;
        for (int k : ks) {
            const int want = limited(d, k);
            if (k >= 0 && k == d - 1) count["k_d_minus_1"]++;
            if (k == d) count["k_d"]++;
            if (k == d + 1) count["k_d_plus_1"]++;
            const int gap = std::abs(Q.m - n);
            if (k >= 0 && gap == k) count["gap_k"]++;
            if (k >= 0 && gap == k + 1) count["gap_k_plus_1"]++;
            for (int pass = 0; pass < (wr ? 2 : 1); pass++) {
                const int cls = pass == 0 ? wr : 0;
                const int got = run_pair(cls, Q, tb, n, k);
                calls++;
                if (got != want && ++mismatches <= 20)
                    printf("MISMATCH kind=%s m=%d n=%d k=%d class=%d got=%d want=%d (d=%d)\n", kind, Q.m, n, k, cls, got,
                           want, d);
            }
        }
    }

    // ---- sequence makers
    Seq rand_seq(int n, const Seq &alpha) {
        Seq s(n, 0);
        for (int i = 0; i < n; i++) s[i] = alpha[rng() % alpha.size()];
        return s;
    }
    int uni(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }   // inclusive
    void edit_at(Seq &s, int pos, const Seq &alpha) {
        if (pos < 0 || pos > (int)s.size()) return;
        const int op = (int)(rng() % 3);
        if (op == 0 && pos < (int)s.size()) s[pos] = alpha[rng() % alpha.size()];
        else if (op == 1) s.insert(s.begin() + pos, alpha[rng() % alpha.size()]);
        else if (pos < (int)s.size()) s.erase(s.begin() + pos);
    }
    Seq mutate(const Seq &s, double rate, const Seq &alpha) {
        Seq out;
        std::uniform_real_distribution<double> U(0.0, 1.0);
        for (char c : s) {
            const double r = U(rng);
            if (r < rate / 3) out.push_back(alpha[rng() % alpha.size()]);
            else if (r < 2 * rate / 3) { out.push_back(c); out.push_back(alpha[rng() % alpha.size()]); }
            else if (r >= rate) out.push_back(c);
        }
        return out;
    }
    Seq alphabet() {
        static const char *bases = "ACGT";
        const int na = uni(2, 4);
        Seq a(bases, bases + na);
        if (rng() % 3 == 0) {   // bytes >= 0x80 (and sometimes 0x00) in the alphabet
            const int nh = uni(1, 3);
            for (int i = 0; i < nh; i++) a.push_back((char)(0x80 + rng() % 128));
            if (rng() % 4 == 0) a.push_back('\0');
        }
        return a;
    }
};

static void print_counts(const Sim &S) {
    for (auto &kv : S.count) printf("%s %lld\n", kv.first.c_str(), kv.second);
    printf("%lld mismatches\n", S.mismatches);
}

static void run_exhaustive() {
    Sim S(1);
    const Seq alpha = "AC";
    for (int m = 1; m <= 6; m++)
        for (int qb = 0; qb < (1 << m); qb++) {
            Seq q(m, 'A');
            for (int i = 0; i < m; i++) q[i] = alpha[(qb >> i) & 1];
            const Query Q(q);
            for (int n = 0; n <= 7; n++) {
                std::vector<int> ks;
                for (int k = -1; k <= std::max(m, n) + 1; k++) ks.push_back(k);
                for (int tb = 0; tb < (1 << n); tb++) {
                    Seq t(n, 'A');
                    for (int j = 0; j < n; j++) t[j] = alpha[(tb >> j) & 1];
                    S.check(Q, t, dp_unlimited(q, t), ks, "exhaustive");
                }
            }
        }
    {   // both empty, and an empty query: the distance is the other side's length, compared with k
        const Query Q0{Seq()};
        for (int n = 0; n <= 3; n++) S.check(Q0, Seq(n, 'A'), n, {-1, 0, n - 1, n, n + 1}, "empty_query");
    }
    printf("pairs %lld\ncalls %lld\n", S.pairs, S.calls);
    print_counts(S);
}

static void run_random(uint64_t seed) {
    Sim S(seed * 0x9E3779B97F4A7C15ull + 11);
    FILE *sample = fopen("oracle_sample.txt", "w");
    if (!sample) { perror("oracle_sample.txt"); exit(2); }
    long long n_sample = 0;
    // query lengths: every register-class and block edge, then random ones up to 1100, then a few long generic ones
    std::vector<int> ms = {1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 767, 768,
                           1023, 1024, 1025, 1087, 1088, 1100};
    for (int i = 0; i < 260; i++) ms.push_back(S.uni(1, 1100));
    for (int i = 0; i < 2; i++) ms.push_back(S.uni(2000, 5000));
    static const char *kinds[] = {"point", "boundary_edits", "indel_start", "indel_end", "gap_k", "identical",
                                  "unrelated"};
    for (int m : ms) {
        const Seq alpha = S.alphabet();
        const Seq q = S.rand_seq(m, alpha);
        const Query Q(q);
        const bool big = m > 1100;
        for (const char *kind : kinds) {
            if (big && strcmp(kind, "point") && strcmp(kind, "indel_start") && strcmp(kind, "indel_end")) continue;
            const std::string K = kind;
            Seq t;
            int gap_k = -2;   // gap_k: a limit equal to the length difference
            if (K == "point") {
                t = S.mutate(q, std::uniform_real_distribution<double>(0.0, 0.15)(S.rng), alpha);
            } else if (K == "boundary_edits") {   // edits on block rows 63/64, 127/128, ... (and the same target columns)
                t = q;
                for (int p = ((int)t.size() - 1) & ~63; p >= 0; p -= 64) {
                    if (S.rng() % 2) S.edit_at(t, p, alpha);
                    if (p > 0 && S.rng() % 2) S.edit_at(t, p - 1, alpha);
                }
            } else if (K == "indel_start" || K == "indel_end") {
                // one long insertion or deletion at the very start or end of either sequence: the band must drop blocks
                // from the top (an insertion in the target shifts the path right) or join them early (a deletion)
                const int len = S.uni(20, 300);
                t = S.mutate(q, 0.02, alpha);
                const bool at_start = K == "indel_start";
                if (S.rng() % 2 || (int)t.size() <= len) t.insert(at_start ? 0 : t.size(), S.rand_seq(len, alpha));
                else t.erase(at_start ? 0 : t.size() - len, len);
            } else if (K == "gap_k") {   // lengths apart by exactly the limit, or one more
                t = S.mutate(q, 0.03, alpha);
                const int len = S.uni(1, 150);
                if (S.rng() % 2 || (int)t.size() <= len) t += S.rand_seq(len, alpha);
                else t.resize(t.size() - len);
                gap_k = std::abs(m - (int)t.size());
            } else if (K == "identical") {
                t = q;
            } else {
                t = S.rand_seq(std::max(0, m + S.uni(-m / 4, 64)), alpha);
            }
            const int d = dp_unlimited(q, t);
            std::vector<int> ks = {-1, d - 1, d, d + 1, (int)(0.1 * m), m, m + 5, S.uni(0, m + 5)};
            if (gap_k >= 0) { ks.push_back(gap_k); ks.push_back(gap_k - 1); }
            S.check(Q, t, d, ks, kind);
            if (m <= 300 && !t.empty() && t.size() <= 400 && S.rng() % 3 == 0) {   // checked against the oracle
                const int k = ks[S.rng() % ks.size()];
                for (unsigned char c : q) fprintf(sample, "%02x", c);
                fprintf(sample, " ");
                for (unsigned char c : t) fprintf(sample, "%02x", c);
                fprintf(sample, " %d %d\n", k, limited(d, k));
                n_sample++;
            }
        }
    }
    fclose(sample);
    printf("pairs %lld\ncalls %lld\noracle_sample %lld\n", S.pairs, S.calls, n_sample);
    print_counts(S);
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "exhaustive")) {
        run_exhaustive();
    } else if (argc >= 3 && !strcmp(argv[1], "random")) {
        run_random(strtoull(argv[2], nullptr, 10));
    } else {
        fprintf(stderr, "usage: pairs_sim exhaustive | random <seed>\n");
        return 2;
    }
    return 0;
}
