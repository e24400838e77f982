// CPU simulation of the specimine kernel's per-pair code (specimux_amd/csrc/smx_mine_core.h): the same host/device
// mine_pair the gfx950 kernel runs, over a Peq table and byte -> row map built the way mine_build_peq builds them in
// LDS, checked against a plain O(mn) DP with edlib's HW semantics.  Every pair runs twice: through the register class
// the host driver would pick for its length, and through the generic class (mine_pair<0>, state in a reused scratch
// slice).  Built and run by tests/test_mine_cpu.py (g++, no GPU).
//
//   mine_sim exhaustive          every {A, C} query of length 1-6 x every {A, C} target of length 0-7 x k = -1..m+1
//   mine_sim random <seed>       structured random cases (see run_random), writes oracle_sample.txt in the cwd
//
// Prints "<counter> <value>" lines (the Python test asserts lower bounds on them) and "<n> mismatches".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "chunk_walk_host.h"   // chunk_with_wr; smx_chunk_plan.h: chunk_class, the state class a call gives a query
#include "smx_mine_core.h"

using namespace smx;
typedef std::string Seq;   // bytes, any value 0x00-0xFF

// edlib HW: the best last-row score over all columns; an empty target costs m whatever k is; -1 if d > k >= 0
static int dp_unlimited(const Seq &q, const Seq &t) {
    const int m = (int)q.size(), n = (int)t.size();
    if (n == 0) return m;
    std::vector<int> col(m + 1);
    for (int i = 0; i <= m; i++) col[i] = i;
    int best = m;
    for (int j = 0; j < n; j++) {
        int diag = 0;   // D[0][j] = 0 (free start)
        const unsigned char c = (unsigned char)t[j];
        for (int i = 1; i <= m; i++) {
            const int up = col[i - 1] + 1, left = col[i] + 1, sub = diag + ((unsigned char)q[i - 1] == c ? 0 : 1);
            diag = col[i];
            col[i] = std::min(std::min(up, left), sub);
        }
        col[0] = 0;
        best = std::min(best, col[m]);
    }
    return best;
}

static int limited(int d, int n, int m, int k) {
    if (n == 0) return m;
    return (k >= 0 && d > k) ? -1 : d;
}

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
                return mine_pair<WR>(st, Q.peq.data(), Q.rowmap, Q.m, Q.W, Q.Wp, k, t, n);
            } else {
                const size_t need = (size_t)Q.W * MINE_THREADS;
                if (sP.size() < need) {   // grow with junk: the kernel's scratch is never initialised either
                    const size_t old = sP.size();
                    sP.resize(need); sM.resize(need); sS.resize(need);
                    for (size_t i = old; i < need; i++) { sP[i] = rng(); sM[i] = rng(); sS[i] = (int)(rng() >> 40); }
                }
                const int lane = (int)(rng() % MINE_THREADS);
                GlobalState st{sP.data() + lane, sM.data() + lane, sS.data() + lane};
                return mine_pair<0>(st, Q.peq.data(), Q.rowmap, Q.m, Q.W, Q.Wp, k, t, n);
            }
        });
    }

    // one (query, target) with every k of ks against the unlimited DP distance d
    void check(const Query &Q, const Seq &q, const Seq &t, int d, const std::vector<int> &ks, const char *kind) {
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
            const int want = limited(d, n, Q.m, k);
            if (n > 0 && k >= 0 && k == d - 1) count["k_d_minus_1"]++;
            if (n > 0 && k == d) count["k_d"]++;
            if (n > 0 && k == d + 1) count["k_d_plus_1"]++;
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

static void run_exhaustive() {
    Sim S(1);
    const Seq alpha = "AC";
    for (int m = 1; m <= 6; m++)
        for (int qb = 0; qb < (1 << m); qb++) {
            Seq q(m, 'A');
            for (int i = 0; i < m; i++) q[i] = alpha[(qb >> i) & 1];
            const Query Q(q);
            std::vector<int> ks;
            for (int k = -1; k <= m + 1; k++) ks.push_back(k);
            for (int n = 0; n <= 7; n++)
                for (int tb = 0; tb < (1 << n); tb++) {
                    Seq t(n, 'A');
                    for (int j = 0; j < n; j++) t[j] = alpha[(tb >> j) & 1];
                    S.check(Q, q, t, dp_unlimited(q, t), ks, "exhaustive");
                }
        }
    printf("pairs %lld\ncalls %lld\n", S.pairs, S.calls);
    for (auto &kv : S.count) printf("%s %lld\n", kv.first.c_str(), kv.second);
    printf("%lld mismatches\n", S.mismatches);
}

static void run_random(uint64_t seed) {
    Sim S(seed * 0x9E3779B97F4A7C15ull + 7);
    FILE *sample = fopen("oracle_sample.txt", "w");
    if (!sample) { perror("oracle_sample.txt"); exit(2); }
    long long n_sample = 0;
    // query lengths: every register-class and block edge, then random ones up to 1100, then a few long generic ones
    std::vector<int> ms = {1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 767, 768,
                           1023, 1024, 1025, 1087, 1088, 1100};
    for (int i = 0; i < 300; i++) ms.push_back(S.uni(1, 1100));
    for (int i = 0; i < 2; i++) ms.push_back(S.uni(2000, 5000));
    static const char *kinds[] = {"point", "boundary_edits", "long_indel", "tandem", "flanked", "unrelated", "short"};
    for (int m : ms) {
        const Seq alpha = S.alphabet();
        const bool tandem = S.rng() % 5 == 0;
        Seq q;
        if (tandem) {   // a tandem repeat query: one unit over and over, lightly mutated
            const Seq unit = S.rand_seq(S.uni(1, 70), alpha);
            while ((int)q.size() < m) q += unit;
            q.resize(m);
            q = S.mutate(q, 0.02, alpha);
            if (q.empty()) q = unit.substr(0, 1);
        } else {
            q = S.rand_seq(m, alpha);
        }
        const Query Q(q);
        const int mq = Q.m;
        const bool big = mq > 1100;
        for (const char *kind : kinds) {
            if (big && strcmp(kind, "point") && strcmp(kind, "long_indel")) continue;   // keep the long ones few
            const std::string K = kind;
            Seq t;
            if (K == "point") {
                t = S.mutate(q, std::uniform_real_distribution<double>(0.0, 0.15)(S.rng), alpha);
            } else if (K == "boundary_edits") {   // edits on block rows 63/64, 127/128, ... (and the same target columns)
                t = q;
                for (int p = ((int)t.size() - 1) & ~63; p >= 0; p -= 64) {
                    if (S.rng() % 2) S.edit_at(t, p, alpha);
                    if (p > 0 && S.rng() % 2) S.edit_at(t, p - 1, alpha);
                }
            } else if (K == "long_indel") {   // one insertion or deletion of 64-300 bytes
                const int len = S.uni(64, 300);
                t = S.mutate(q, 0.02, alpha);
                const int pos = S.uni(0, (int)t.size());
                if (S.rng() % 2 || (int)t.size() <= len) t.insert(pos, S.rand_seq(len, alpha));
                else t.erase(std::min(pos, (int)t.size() - len), len);
            } else if (K == "tandem") {   // a repeat of a piece of the query, with a different copy number
                const int ul = S.uni(1, std::min(mq, 70));
                const Seq unit = q.substr(S.uni(0, mq - ul), ul);
                const int len = std::max(0, mq + S.uni(-mq / 4, mq / 4 + 64));
                while ((int)t.size() < len) t += unit;
                t = S.mutate(t.substr(0, len), 0.03, alpha);
            } else if (K == "flanked") {
                t = S.rand_seq(S.uni(0, 200), alpha) + S.mutate(q, 0.05, alpha) + S.rand_seq(S.uni(0, 200), alpha);
            } else if (K == "unrelated") {
                t = S.rand_seq(std::max(0, mq + S.uni(-mq / 4, 64)), alpha);
            } else {   // shorter than m - k for the usual limits
                t = S.mutate(q, 0.05, alpha);
                t.resize(std::min(t.size(), (size_t)S.uni(0, std::max(0, (int)(0.85 * mq) - 1))));
            }
            const int d = dp_unlimited(q, t);
            std::vector<int> ks = {-1, d - 1, d, d + 1, (int)(0.15 * mq), mq, mq + 5, S.uni(0, mq + 5)};
            S.check(Q, q, t, d, ks, kind);
            if (mq <= 300 && t.size() <= 400 && S.rng() % 3 == 0) {   // the Python test checks these against the oracle
                const int k = ks[S.rng() % ks.size()];
                for (unsigned char c : q) fprintf(sample, "%02x", c);
                fprintf(sample, " ");
                for (unsigned char c : t) fprintf(sample, "%02x", c);
                fprintf(sample, "%s %d %d\n", t.empty() ? "-" : "", k, limited(d, (int)t.size(), mq, k));
                n_sample++;
            }
        }
    }
    fclose(sample);
    printf("pairs %lld\ncalls %lld\noracle_sample %lld\n", S.pairs, S.calls, n_sample);
    for (auto &kv : S.count) printf("%s %lld\n", kv.first.c_str(), kv.second);
    printf("%lld mismatches\n", S.mismatches);
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "exhaustive")) {
        run_exhaustive();
    } else if (argc >= 3 && !strcmp(argv[1], "random")) {
        run_random(strtoull(argv[2], nullptr, 10));
    } else {
        fprintf(stderr, "usage: mine_sim exhaustive | random <seed>\n");
        return 2;
    }
    return 0;
}
