// CPU simulation of the consensus kernel's per-pair code (specimux_amd/csrc/smx_cons_core.h): the same host/device
// cons_pair the gfx950 kernel runs, over a Peq table and byte -> row map built the way mine_build_peq builds them in
// LDS, checked against a plain O(mn) DP whose full matrix is walked back by the same fixed rule (diagonal, else up, else
// left).  Distances and pileup rows must be identical word for word.  Every pair runs twice: through the register class
// the host driver would pick for the draft's length, and through the generic class (state in a reused scratch slice).
// The history is a reused, never cleared slice with the lane stride of the kernel, sized by cons_band_blocks exactly
// or with slack.  Built and run by tests/test_cons_cpu.py (g++, no GPU).
//
//   cons_sim exhaustive         every {A, C} draft of length 1-6 x every {A, C} read of length 0-7 x
//                               k = -1..max(m, n) + 1
//   cons_sim random <seed>      structured random cases (see run_random), writes oracle_sample.txt in the cwd
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

#include "chunk_walk_host.h"   // chunk_with_wr; smx_chunk_plan.h: chunk_class, the state class a call gives a draft
#include "smx_cons_core.h"

using namespace smx;
typedef std::string Seq;   // bytes, any value 0x00-0xFF

static unsigned code_of(unsigned char c) {
    switch (c) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
        default: return 4;
    }
}

// NW over the full matrix (D[i][0] = i, D[0][j] = j), then the walk from (m, n).  Returns D[m][n].
static int dp_row(const Seq &q, const Seq &t, std::vector<uint32_t> *row_out) {
    const int m = (int)q.size(), n = (int)t.size();
    std::vector<int> D((size_t)(m + 1) * (n + 1));
    auto at = [&](int i, int j) -> int & { return D[(size_t)i * (n + 1) + j]; };
    for (int i = 0; i <= m; i++) at(i, 0) = i;
    for (int j = 0; j <= n; j++) at(0, j) = j;
    for (int i = 1; i <= m; i++)
        for (int j = 1; j <= n; j++)
            at(i, j) = std::min(std::min(at(i - 1, j) + 1, at(i, j - 1) + 1), at(i - 1, j - 1) + (q[i - 1] != t[j - 1]));
    std::vector<uint32_t> &row = *row_out;
    row.assign(m + 1, 0);
    std::vector<unsigned> sym(m + 1, 7), ilen(m + 1, 0);
    std::vector<std::vector<unsigned>> ins(m + 1);   // inserted codes before position p, collected backwards
    int i = m, j = n;
    while (i > 0 || j > 0) {
        if (i > 0 && j > 0 && at(i - 1, j - 1) + (q[i - 1] != t[j - 1]) == at(i, j)) {
            sym[i - 1] = code_of((unsigned char)t[j - 1]);
            i--, j--;
        } else if (i > 0 && at(i - 1, j) + 1 == at(i, j)) {
            sym[i - 1] = 5;
            i--;
        } else {
            ins[i].push_back(code_of((unsigned char)t[j - 1]));
            ilen[i]++;
            j--;
        }
    }
    for (int p = 0; p <= m; p++) {
        std::reverse(ins[p].begin(), ins[p].end());   // read order
        uint32_t w = sym[p] | (std::min(ilen[p], 255u) << 3);
        for (size_t s = 0; s < ins[p].size() && s < SMX_CONS_MAX_INS; s++) w |= ins[p][s] << (11 + 3 * s);
        row[p] = w;
    }
    return at(m, n);
}

static int limited(int d, int k) { return (k >= 0 && d > k) ? -1 : d; }

// The draft as the kernel sees it in LDS: rows 1..nrows for its distinct bytes in byte order, row 0 all zero.
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

static int reg_class(int W) { return CHUNK_CLASS_WORDS[chunk_class((size_t)W)]; }

struct Sim {
    std::mt19937_64 rng;
    std::vector<u64> sP, sM;          // generic-class scratch, [word][lane], reused from pair to pair
    std::vector<int> sS;
    std::vector<cons_pm> hPM;         // the history slice, [column][slot][lane], reused from pair to pair
    std::vector<int> hS;
    std::vector<mine_u4> tbuf;
    std::vector<uint32_t> want_row, got_row;
    long long pairs = 0, calls = 0, mismatches = 0;
    std::map<std::string, long long> count;

    explicit Sim(uint64_t seed) : rng(seed) {}

    int run_pair(int wr, const Query &Q, const unsigned char *t, int n, int k, uint32_t *row) {
        const int lane = (int)(rng() % MINE_THREADS);
        const int B = cons_band_blocks(Q.m, n, k) + (int)(rng() % 2);   // exactly what the band needs, or one more
        const size_t need = (size_t)n * B * MINE_THREADS;
        if (hPM.size() < need) {       // grow with junk: the kernel's workspace is never initialised either
            const size_t old = hPM.size();
            hPM.resize(need); hS.resize(need);
            for (size_t i = old; i < need; i++) { hPM[i] = cons_pm{rng(), rng()}; hS[i] = (int)(rng() >> 40); }
        }
        const ConsHist H{hPM.data() + lane, hS.data() + lane, B};
        return chunk_with_wr(wr, [&](auto WR) {
            if constexpr (WR > 0) {
                RegState<WR> st;
                return cons_pair<WR>(st, H, Q.peq.data(), Q.rowmap, Q.m, Q.W, Q.Wp, k, t, n, row);
            } else {
                const size_t sneed = (size_t)std::max(Q.W, 1) * MINE_THREADS;
                if (sP.size() < sneed) {
                    const size_t old = sP.size();
                    sP.resize(sneed); sM.resize(sneed); sS.resize(sneed);
                    for (size_t i = old; i < sneed; i++) { sP[i] = rng(); sM[i] = rng(); sS[i] = (int)(rng() >> 40); }
                }
                GlobalState st{sP.data() + lane, sM.data() + lane, sS.data() + lane};
                return cons_pair<0>(st, H, Q.peq.data(), Q.rowmap, Q.m, Q.W, Q.Wp, k, t, n, row);
            }
        });
    }

    // what a row must satisfy by itself: replayed on the draft it rebuilds the read (no insertion longer than the
    // slots), and its edits add up to the distance (no insertion longer than the length field)
    void check_row(const Seq &q, const Seq &t, int d, const char *kind) {
        static const char letters[4] = {'A', 'C', 'G', 'T'};
        const int m = (int)q.size();
        for (unsigned char c : t)
            if (code_of(c) > 3) return;            // a symbol "other" hides which byte it was
        bool replay_ok = true, count_ok = true;
        Seq rebuilt;
        long long edits = 0;
        for (int p = 0; p <= m; p++) {
            const uint32_t w = want_row[p];
            const unsigned len = (w >> 3) & 255u, s = w & 7u;
            if (len == 255u) count_ok = false;
            if (len > SMX_CONS_MAX_INS) replay_ok = false;
            edits += len;
            for (unsigned x = 0; x < std::min(len, (unsigned)SMX_CONS_MAX_INS); x++) rebuilt.push_back(letters[(w >> (11 + 3 * x)) & 3u]);
            if (p == m) {
                if (s != 7u && ++mismatches <= 20) printf("ROW kind=%s: word m has symbol %u\n", kind, s);
            } else if (s == 5u) {
                edits++;
            } else {
                rebuilt.push_back(letters[s & 3u]);
                edits += letters[s & 3u] != q[p];
            }
        }
        if (replay_ok) {
            count["replayed"]++;
            if (rebuilt != t && ++mismatches <= 20) printf("REPLAY kind=%s m=%d n=%d differs\n", kind, m, (int)t.size());
        }
        if (count_ok) {
            count["edit_counted"]++;
            if (edits != d && ++mismatches <= 20) printf("EDITS kind=%s m=%d n=%d edits=%lld d=%d\n", kind, m, (int)t.size(), edits, d);
        }
    }

    // one (draft, read) with every k of ks against the full-matrix DP
    // (want_row and d come from reference(q, t))
    int reference(const Seq &q, const Seq &t) { return dp_row(q, t, &want_row); }

    void check(const Seq &q, const Query &Q, const Seq &t, int d, const std::vector<int> &ks, const char *kind) {
        const int n = (int)t.size();
        check_row(q, t, d, kind);
        tbuf.assign((size_t)n / 16 + 1, mine_u4{0, 0, 0, 0});
        unsigned char *tb = reinterpret_cast<unsigned char *>(tbuf.data());
        for (size_t i = n; i < tbuf.size() * 16; i++) tb[i] = (unsigned char)rng();
        memcpy(tb, t.data(), (size_t)n);
        pairs++;
        count[std::string("kind_") + kind]++;
        const int wr = reg_class(Q.W);
        count["class_" + std::to_string(wr)]++;
        for (unsigned x = 0; x <= (unsigned)Q.m; x++) {
            const unsigned len = (want_row[x] >> 3) & 255u;
            if (len == SMX_CONS_MAX_INS) count["ins_len_4"]++;
            if (len == SMX_CONS_MAX_INS + 1) count["ins_len_5"]++;
            if (len == 255u) count["ins_len_clipped"]++;
        }
        for (int k : ks) {
            const int want = limited(d, k);
            if (k >= 0 && k == d - 1) count["k_d_minus_1"]++;
            if (k == d) count["k_d"]++;
            if (k == d + 1) count["k_d_plus_1"]++;
            const int gap = std::abs(Q.m - n);
            if (k >= 0 && gap == k) count["gap_k"]++;
            if (k >= 0 && gap == k + 1) count["gap_k_plus_1"]++;
            if (want >= 0 && Q.m > 0 && n > 0) {    // what the band did on the way: blocks dropped at the top, joined at the bottom
                const int big = std::max(Q.m, n), kk = (k < 0 || k > big) ? big : k, g = Q.m - n, ag = std::abs(g);
                const int e = (kk - ag) >> 1, dlo = std::min(g, 0) - e, dhi = std::max(g, 0) + e;
                if (n - 1 + dlo >= 64) count["band_top_dropped"]++;
                if ((dhi >> 6) < Q.W - 1) count["band_bottom_joined"]++;
            }
            for (int pass = 0; pass < (wr ? 2 : 1); pass++) {
                const int cls = pass == 0 ? wr : 0;
                got_row.assign((size_t)Q.m + 1, 0xA5A5A5A5u);
                const int got = run_pair(cls, Q, tb, n, k, got_row.data());
                calls++;
                if (got != want) {
                    if (++mismatches <= 20)
                        printf("MISMATCH kind=%s m=%d n=%d k=%d class=%d got=%d want=%d (d=%d)\n", kind, Q.m, n, k, cls, got, want, d);
                } else if (want >= 0 && got_row != want_row) {
                    if (++mismatches <= 20) {
                        size_t p = 0;
                        while (got_row[p] == want_row[p]) p++;
                        printf("ROW MISMATCH kind=%s m=%d n=%d k=%d class=%d d=%d word %zu: got %08x want %08x\n", kind, Q.m, n, k,
                               cls, d, p, got_row[p], want_row[p]);
                    }
                } else if (want >= 0) {
                    count["rows_equal"]++;
                }
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
        if (rng() % 3 == 0) {   // bytes >= 0x80 (and sometimes 0x00) in the alphabet: symbol "other"
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
                    S.check(q, Q, t, S.reference(q, t), ks, "exhaustive");
                }
            }
        }
    printf("pairs %lld\ncalls %lld\n", S.pairs, S.calls);
    print_counts(S);
}

static void run_random(uint64_t seed) {
    Sim S(seed * 0x9E3779B97F4A7C15ull + 17);
    FILE *sample = fopen("oracle_sample.txt", "w");
    if (!sample) { perror("oracle_sample.txt"); exit(2); }
    long long n_sample = 0;
    // draft lengths: every register-class and block edge, then random ones up to 1100, then two long generic ones
    std::vector<int> ms = {1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 767, 768,
                           1023, 1024, 1025, 1087, 1088, 1100};
    for (int i = 0; i < 150; i++) ms.push_back(S.uni(1, 1100));
    for (int i = 0; i < 2; i++) ms.push_back(S.uni(1500, 2500));
    static const char *kinds[] = {"point", "boundary_edits", "indel_start", "indel_end", "gap_k", "identical", "unrelated",
                                  "ins_clip", "homopolymer", "band_top"};
    for (int m : ms) {
        const Seq alpha = S.alphabet();
        const Seq q = S.rand_seq(m, alpha);
        const Query Q(q);
        const bool big = m > 1100;
        for (const char *kind : kinds) {
            if (big && strcmp(kind, "point") && strcmp(kind, "indel_start") && strcmp(kind, "indel_end") && strcmp(kind, "band_top"))
                continue;
            const std::string K = kind;
            Seq t;
            const Seq *draft = &q;
            Seq q2;
            int gap_k = -2;
            if (K == "point") {
                t = S.mutate(q, std::uniform_real_distribution<double>(0.0, 0.15)(S.rng), alpha);
            } else if (K == "boundary_edits") {   // edits on block rows 63 / 64 / 65, 127 / 128 / 129, ...
                t = q;
                for (int p = ((int)t.size() - 1) & ~63; p >= 0; p -= 64) {
                    if (S.rng() % 2) S.edit_at(t, p + 1, alpha);
                    if (S.rng() % 2) S.edit_at(t, p, alpha);
                    if (p > 0 && S.rng() % 2) S.edit_at(t, p - 1, alpha);
                }
            } else if (K == "indel_start" || K == "indel_end") {
                const int len = S.uni(20, 300);
                t = S.mutate(q, 0.02, alpha);
                const bool at_start = K == "indel_start";
                if (S.rng() % 2 || (int)t.size() <= len) t.insert(at_start ? 0 : t.size(), S.rand_seq(len, alpha));
                else t.erase(at_start ? 0 : t.size() - len, len);
            } else if (K == "gap_k") {
                t = S.mutate(q, 0.03, alpha);
                const int len = S.uni(1, 150);
                if (S.rng() % 2 || (int)t.size() <= len) t += S.rand_seq(len, alpha);
                else t.resize(t.size() - len);
                gap_k = std::abs(m - (int)t.size());
            } else if (K == "identical") {
                t = q;
            } else if (K == "unrelated") {
                t = S.rand_seq(std::max(0, m + S.uni(-m / 4, 64)), alpha);
            } else if (K == "ins_clip") {         // insertions of 4, 5 and 300 bases: the slot clip and the length clip
                t = q;
                static const int lens[3] = {4, 5, 300};
                for (int len : lens) t.insert(S.uni(0, (int)t.size()), S.rand_seq(len, alpha));
            } else if (K == "homopolymer") {      // a run in the draft, one base short in the read
                const int run = S.uni(3, 12), at = S.uni(0, m);
                q2 = q;
                q2.insert(at, Seq(run, alpha[S.rng() % alpha.size()]));
                t = q2;
                t.erase(at + S.uni(0, run - 1), 1);
                draft = &q2;
            } else {                              // band_top: few edits, so that the small limits keep a narrow band
                t = S.mutate(q, 0.01, alpha);
            }
            const int d = S.reference(*draft, t);
            if (draft != &q) {
                S.check(*draft, Query(*draft), t, d, {-1, d - 1, d, d + 1, (int)(0.1 * m), S.uni(0, m + 5)}, kind);
                continue;
            }
            if (big) {                            // limited pairs only: the history of a full matrix of this size is large
                S.check(q, Q, t, d, {d - 1, d, d + 1, d + 40}, kind);
                continue;
            }
            std::vector<int> ks = {-1, d - 1, d, d + 1, (int)(0.1 * m), m, m + 5, S.uni(0, m + 5)};
            if (gap_k >= 0) { ks.push_back(gap_k); ks.push_back(gap_k - 1); }
            S.check(q, Q, t, d, ks, kind);
            if (m <= 300 && !t.empty() && t.size() <= 400 && S.rng() % 2 == 0) {   // checked against the oracle
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
        fprintf(stderr, "usage: cons_sim exhaustive | random <seed>\n");
        return 2;
    }
    return 0;
}
