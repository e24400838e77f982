// CPU simulation of the bit-sliced barcode scans of the demux kernel's lean mode (specimux_amd/csrc/smx_barcode_core.h):
// the same host/device bitsliced_shw, bitsliced_shw_pad and bitsliced_shw_pad_tails the gfx950 kernel runs, over table
// blocks filled by the product's bs_table_add, checked barcode by barcode against a plain O(mn) SHW DP with IUPAC
// equality.  Every instantiation the kernel has runs at every barcode length m it can hold (not only the m the kernel's
// dispatch picks) and every k from 0 to min(KB, m - 1).  Built and run by tests/test_barcode_scan_cpu.py (g++, no GPU;
// once more with -fsanitize=address,undefined: table blocks are exactly 256 words and target buffers exactly as long as
// the bytes the kernel's LDS layout guarantees behind a target, so a read past either fails).
//
//   barcode_sim exhaustive [mmax] every {A, C} barcode of length m = 1..mmax (default 5) in one word x every target over
//                                {C, N, R, code 15} ({N, R, code 15} at m = 5) of every length 0 .. m + KB + 1
//   barcode_sim random <seed>    structured random cases (see run_random), writes oracle_sample.txt in the cwd
//
// Prints "<counter> <value>" lines (the Python test asserts lower bounds on them) and "<n> mismatches".
//
// What is exact, per call (kidx = k):
//   bitsliced_shw<8>            seen[d], d <= k: exactly the barcodes whose last DP row holds d at some column 1..ncol
//   bitsliced_shw_pad<KB, M>    the lowest level <= k holding a barcode's bit is its minimum over row m when that is
//                               <= k; no bit at levels <= k otherwise.  Levels above the minimum may hold extra bits:
//                               row M away from the minimum's diagonal is not row m (it reaches the minimum's columns
//                               only by paying horizontal steps), and the lean summary only reads the lowest level.
//   bitsliced_shw_pad_tails     seen as bitsliced_shw_pad; ML[d] = the barcodes whose minimum is d (<= k); tailcol = the
//                               last column x < ncol at which a barcode of ML[d] & want[d] has D[m][x + 1] == d
//   all                         no bit of a barcode slot the word does not hold at any level <= k
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "smx_barcode_core.h"

using namespace smx;

static const char kCodes[] = "ACGTNRYKMSWBDHV";   // text codes 0..14 (smx_internal.h kCodeChars); 15 matches nothing
static const int INF = 1 << 20;

// IUPAC equality (28 symmetric pairs, not transitive) on letters
static bool iupac_eq(char a, char b) {
    if (a == b) return true;
    static const char *pairs[] = {"YC", "YT", "RA", "RG", "NA", "NC", "NG", "NT", "WA", "WT", "MA", "MC", "SC", "SG",
                                  "KG", "KT", "BC", "BG", "BT", "DA", "DG", "DT", "HA", "HC", "HT", "VA", "VC", "VG"};
    for (const char *p : pairs)
        if ((p[0] == a && p[1] == b) || (p[0] == b && p[1] == a)) return true;
    return false;
}
struct EqCode {   // [barcode letter][text code]
    bool t[128][16];
    EqCode() {
        for (int a = 0; a < 128; a++)
            for (int c = 0; c < 16; c++) t[a][c] = c < 15 && iupac_eq((char)a, kCodes[c]);
    }
};
static const EqCode eqc;
static bool eq_code(char bc, int code) { return eqc.t[(unsigned char)bc & 127][code]; }

// SHW: D[0][j] = j, D[i][0] = i; returns D[m][j] for j = 0..n
static std::vector<int> dp_last_row(const std::string &b, const std::vector<int> &t) {
    const int m = (int)b.size(), n = (int)t.size();
    std::vector<int> prev(m + 1), cur(m + 1), last(n + 1);
    for (int i = 0; i <= m; i++) prev[i] = i;
    last[0] = m;
    for (int j = 1; j <= n; j++) {
        cur[0] = j;
        for (int i = 1; i <= m; i++)
            cur[i] = std::min(std::min(prev[i] + 1, cur[i - 1] + 1), prev[i - 1] + (eq_code(b[i - 1], t[j - 1]) ? 0 : 1));
        last[j] = cur[m];
        std::swap(prev, cur);
    }
    return last;
}

// The kernel's choice of scan for a uniform barcode length bsm (smx_demux_tile.h phase3b_barcodes / phase3c_summary, the
// if-chains at the bitsliced_shw* calls): k <= 3 -> pad<3, 13> if bsm == 13, <3, 8> for 4..8, <3, 12> for 9..12, else
// <3, 16>; k = 4 -> pad<4, 13> if bsm == 13, else <4, 16>; k 5..7 -> bitsliced_shw<8>.  Restated here, not shared, so
// that the kernel's instructions stay as they were.
static int dispatched_M(int kidx, int bsm) {
    if (kidx <= 3) return bsm == 13 ? 13 : (bsm <= 8 && bsm > 3) ? 8 : (bsm <= 12 && bsm > 3) ? 12 : 16;
    if (kidx == 4 && bsm > 4 && bsm <= 16) return bsm == 13 ? 13 : 16;
    return 0;
}

struct Word {
    int m = 0;
    std::vector<std::string> bc;   // <= 32, all of length m
    std::vector<std::array<unsigned, 16>> peq;
};

static Word make_word(const std::vector<std::string> &bcs) {
    Word w;
    w.m = (int)bcs[0].size();
    w.bc = bcs;
    for (const auto &b : bcs) {
        std::array<unsigned, 16> p{};
        for (int c = 0; c < 16; c++)
            for (int i = 0; i < (int)b.size(); i++)
                if (eq_code(b[i], c)) p[c] |= 1u << i;
        w.peq.push_back(p);
    }
    return w;
}

static std::map<std::string, long> counters;
static long mismatches = 0;
static std::mt19937_64 junk_rng(12345);

#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            if (++mismatches <= 20) {                                                     \
                fprintf(stdout, "MISMATCH %s:%d (%s) ", inst, __LINE__, #cond);           \
                fprintf(stdout, __VA_ARGS__);                                             \
                fprintf(stdout, "\n");                                                    \
            }                                                                             \
        }                                                                                 \
    } while (0)

// the DP view of one (word, target) pair
struct Ref {
    int nb, ncol;
    std::vector<std::vector<int>> last;   // [b][j]
    std::vector<int> mn;                  // min over j = 1..ncol (INF if ncol == 0)
    unsigned level(int d) const {         // barcodes with D[m][j] == d at some j in 1..ncol
        unsigned s = 0;
        for (int b = 0; b < nb; b++)
            for (int j = 1; j <= ncol; j++)
                if (last[b][j] == d) { s |= 1u << b; break; }
        return s;
    }
    int lastcol(int b, int d) const {     // the largest x < ncol with D[m][x + 1] == d, -1 if none
        for (int x = ncol - 1; x >= 0; x--)
            if (last[b][x + 1] == d) return x;
        return -1;
    }
};

static Ref make_ref(const Word &w, const std::vector<int> &t) {
    Ref r;
    r.nb = (int)w.bc.size();
    r.ncol = (int)t.size();
    for (int b = 0; b < r.nb; b++) {
        r.last.push_back(dp_last_row(w.bc[b], t));
        int mn = INF;
        for (int j = 1; j <= r.ncol; j++) mn = std::min(mn, r.last[b][j]);
        r.mn.push_back(mn);
    }
    return r;
}

// the table block of one word, exactly 256 words, filled by the product's code
static std::unique_ptr<unsigned[]> make_block(const Word &w) {
    std::unique_ptr<unsigned[]> blk(new unsigned[256]);
    for (int i = 0; i < 256; i++) blk[i] = 0u;
    for (int b = 0; b < (int)w.bc.size(); b++) bs_table_add(blk.get(), b, w.peq[b].data(), w.m);
    return blk;
}

// a target buffer of exactly `bytes` bytes: the target's codes, then junk (any byte) up to the end
static std::unique_ptr<unsigned char[]> make_target(const std::vector<int> &t, int bytes) {
    std::unique_ptr<unsigned char[]> buf(new unsigned char[bytes]);
    for (int i = 0; i < bytes; i++) buf[i] = i < (int)t.size() ? (unsigned char)t[i] : (unsigned char)(junk_rng() & 0xFF);
    return buf;
}

static unsigned word_mask(int nb) { return nb >= 32 ? ~0u : ((1u << nb) - 1u); }

// the per-barcode minimum the levels of one call report: the lowest level <= k holding the bit, INF if none
template <int NL>
static int lowest(const unsigned (&seen)[NL], int b, int kidx) {
    for (int d = 0; d <= kidx && d < NL; d++)
        if ((seen[d] >> b) & 1u) return d;
    return INF;
}

// one hit: the OR of its entries' levels (phase 3c's dmask) and what the summary makes of it
struct Hit {
    unsigned dm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

static void check_summary(const char *inst, const Hit &h, const std::vector<Ref> &refs, int kidx) {
    // phase 3c: best = lowest non-empty level <= k, ntied = its popcount, first_tied = its first bit
    int best = -1, ntied = 0, first = -1;
    for (int d = 0; d <= kidx; d++)
        if (h.dm[d]) { best = d; ntied = __builtin_popcount(h.dm[d]); first = __builtin_ctz(h.dm[d]); break; }
    int rb = INF, rn = 0, rf = -1;
    const int nb = refs[0].nb;
    for (int b = 0; b < nb; b++) {
        int mb = INF;
        for (const Ref &r : refs) mb = std::min(mb, r.mn[b]);
        if (mb > kidx) continue;
        if (mb < rb) { rb = mb; rn = 0; rf = b; }
        if (mb == rb) rn++;
    }
    if (rb == INF) rb = -1, rf = -1;
    CHECK(best == rb && ntied == rn && first == rf, "summary k=%d best %d/%d ntied %d/%d first %d/%d", kidx, best, rb, ntied, rn, first, rf);
    counters["summary_hits"]++;
    if (rn >= 2) counters["summary_ties"]++;
    if (rb == kidx) counters["summary_best_eq_k"]++;
    if (rb < 0) counters["summary_none"]++;
    if (refs.size() > 1) counters["summary_multi_entry"]++;
}

template <int KB, int M>
static void run_pad(const char *inst, const Word &w, const unsigned *blk, const std::vector<std::vector<int>> &targets,
                    const std::vector<Ref> &refs, int kidx, std::mt19937_64 &rng, bool tails, const std::vector<int> &offs) {
    const int m = w.m, nb = (int)w.bc.size();
    const unsigned live = word_mask(nb);
    Hit hit;
    std::vector<std::array<unsigned, KB + 1>> seens;
    for (size_t e = 0; e < targets.size(); e++) {
        const Ref &r = refs[e];
        auto buf = make_target(targets[e], M + KB);
        unsigned seen[KB + 1];
        bitsliced_shw_pad<KB, M>(blk, buf.get(), r.ncol, m, kidx, seen);
        for (int b = 0; b < nb; b++) {
            const int want = r.mn[b] <= kidx ? r.mn[b] : INF;
            CHECK(lowest(seen, b, kidx) == want, "m=%d k=%d ncol=%d b=%d lowest %d dp %d", m, kidx, r.ncol, b, lowest(seen, b, kidx), r.mn[b]);
            if (r.mn[b] == kidx) counters["min_eq_k"]++;
            if (r.mn[b] == kidx + 1) counters["min_eq_k_plus_1"]++;
        }
        for (int d = 0; d <= kidx; d++) CHECK((seen[d] & ~live) == 0, "m=%d k=%d level %d: bits of missing barcodes %08x", m, kidx, d, seen[d] & ~live);
        for (int d = 0; d <= kidx; d++) hit.dm[d] |= seen[d];
        std::array<unsigned, KB + 1> sa;
        for (int d = 0; d <= KB; d++) sa[d] = seen[d];
        seens.push_back(sa);
        if (tails) {   // the tails variant on the same input, with a random want per level (all ones included)
            unsigned want[KB + 1], s2[KB + 1], ML[KB + 1];
            const bool allones = rng() % 4 == 0;
            for (int d = 0; d <= KB; d++) {
                const int pick = (int)(rng() % 4);
                want[d] = allones || pick == 0 ? ~0u : pick == 1 ? (unsigned)rng() : pick == 2 ? 0u : (unsigned)(rng() & rng());
            }
            int tc = 12345;
            auto buf2 = make_target(targets[e], M + KB);
            bitsliced_shw_pad_tails<KB, M>(blk, buf2.get(), r.ncol, m, kidx, want, s2, ML, tc);
            for (int d = 0; d <= KB; d++) CHECK(s2[d] == seen[d], "tails seen m=%d k=%d d=%d %08x vs %08x", m, kidx, d, s2[d], seen[d]);
            int rt = -1;
            for (int d = 0; d <= KB; d++) {
                unsigned rml = 0;
                if (d <= kidx)
                    for (int b = 0; b < nb; b++)
                        if (r.mn[b] == d) rml |= 1u << b;
                CHECK(ML[d] == rml, "ML m=%d k=%d d=%d %08x vs %08x", m, kidx, d, ML[d], rml);
                for (int b = 0; b < nb; b++)
                    if (((rml & want[d]) >> b) & 1u) rt = std::max(rt, r.lastcol(b, d));
            }
            CHECK(tc == rt, "tailcol m=%d k=%d ncol=%d %d vs %d", m, kidx, r.ncol, tc, rt);
            counters[allones ? "tails_want_all" : "tails_want_partial"]++;
            if (rt >= 0) counters["tails_col_found"]++;
        }
    }
    check_summary(inst, hit, refs, kidx);
    if (tails) {   // phase 3c's tails pass over the hit's entries: want = GM & ~prev, the first entry at each barcode's best
        unsigned GM[KB + 1], prev[KB + 1], lower = 0;
        for (int d = 0; d <= KB; d++) {
            GM[d] = d <= kidx ? (hit.dm[d] & ~lower) : 0u;
            lower |= d <= kidx ? hit.dm[d] : 0u;
            prev[d] = 0u;
        }
        int t = -INF;
        for (size_t e = 0; e < targets.size(); e++) {
            unsigned want[KB + 1], s2[KB + 1], ML[KB + 1];
            unsigned anyw = 0;
            for (int d = 0; d <= KB; d++) { want[d] = GM[d] & ~prev[d]; anyw |= want[d]; }
            if (!anyw) break;
            auto buf = make_target(targets[e], M + KB);
            int tc = -1;
            bitsliced_shw_pad_tails<KB, M>(blk, buf.get(), refs[e].ncol, m, kidx, want, s2, ML, tc);
            if (tc >= 0) t = std::max(t, offs[e] + tc);
            for (int d = 0; d <= KB; d++) prev[d] |= ML[d] & GM[d];
        }
        int rt = -INF;
        for (int b = 0; b < nb; b++) {
            int mb = INF;
            for (const Ref &r : refs) mb = std::min(mb, r.mn[b]);
            if (mb > kidx) continue;
            for (size_t e = 0; e < refs.size(); e++)
                if (refs[e].mn[b] == mb) { rt = std::max(rt, offs[e] + refs[e].lastcol(b, mb)); break; }
        }
        CHECK(t == rt, "hit tail m=%d k=%d entries=%d %d vs %d", m, kidx, (int)targets.size(), t, rt);
    }
    counters[std::string("calls_") + inst + "_k" + std::to_string(kidx)] += (long)targets.size();
    if (dispatched_M(kidx, m) == M && (KB == 3) == (kidx <= 3)) counters["calls_dispatched"] += (long)targets.size();
}

static void run_shw8(const char *inst, const Word &w, const unsigned *blk, const std::vector<std::vector<int>> &targets,
                     const std::vector<Ref> &refs, int kidx) {
    const int m = w.m, nb = (int)w.bc.size();
    Hit hit;
    for (size_t e = 0; e < targets.size(); e++) {
        const Ref &r = refs[e];
        auto buf = make_target(targets[e], m + kidx);   // the scan reads cw[c] for c < min(ncol, m + k) only
        unsigned seen[8];
        bitsliced_shw<8>(blk, buf.get(), r.ncol, m, kidx, seen);
        for (int d = 0; d < 8; d++) {
            const unsigned want = d <= kidx ? r.level(d) : 0u;
            CHECK(seen[d] == want, "m=%d k=%d ncol=%d level %d: %08x vs %08x", m, kidx, r.ncol, d, seen[d], want);
        }
        for (int b = 0; b < nb; b++) {
            if (r.mn[b] == kidx) counters["min_eq_k"]++;
            if (r.mn[b] == kidx + 1) counters["min_eq_k_plus_1"]++;
        }
        for (int d = 0; d <= kidx; d++) hit.dm[d] |= seen[d];
    }
    check_summary(inst, hit, refs, kidx);
    counters[std::string("calls_") + inst + "_k" + std::to_string(kidx)] += (long)targets.size();
    if (dispatched_M(kidx, m) == 0 && kidx >= 4) counters["calls_dispatched"] += (long)targets.size();
}

// every instantiation the kernel has, at every k it can run this word with; `maxlen` (exhaustive mode) limits each
// instantiation to targets of length <= m + KB + 1
static void run_all(const Word &w, const std::vector<std::vector<int>> &targets, std::mt19937_64 &rng, const std::vector<int> &offs,
                    bool limit_len) {
    const int m = w.m;
    auto blk = make_block(w);
    std::vector<Ref> refs;
    for (const auto &t : targets) refs.push_back(make_ref(w, t));
    int tmax = 0;
    for (const auto &t : targets) tmax = std::max(tmax, (int)t.size());
    if ((int)w.bc.size() < 32) counters["partial_word_hits"]++;
#define PAD(KB, M, T)                                                                                                   \
    if (m <= M && (!limit_len || tmax <= m + KB + 1))                                                                  \
        for (int k = 0; k <= std::min(KB, m - 1); k++)                                                                 \
            run_pad<KB, M>(T ? "tails" #KB "_" #M : "pad" #KB "_" #M, w, blk.get(), targets, refs, k, rng, T, offs);
    PAD(3, 8, false) PAD(3, 12, false) PAD(3, 13, false) PAD(3, 16, false)
    PAD(4, 13, false) PAD(4, 16, false)
    PAD(3, 8, true) PAD(3, 12, true) PAD(3, 13, true) PAD(3, 16, true)
#undef PAD
    for (int k = 0; k <= std::min(7, m - 1); k++)
        if (!limit_len || tmax <= m + k + 1) run_shw8("shw8", w, blk.get(), targets, refs, k);
}

static void run_exhaustive(int mmax) {
    // C, N, R, code 15: against {A, C} barcodes every subset of {A, C} matches.  The full word (m = 5) runs over N, R and
    // code 15 only, which keeps the run short; the 32 barcodes still see every column pattern R makes of them.
    const int alpha[4] = {4, 5, 15, 1};
    for (int m = 1; m <= mmax; m++) {
        const int na = m <= 4 ? 4 : 3;
        std::vector<std::string> bcs;
        for (int x = 0; x < (1 << m); x++) {
            std::string b;
            for (int i = 0; i < m; i++) b += ((x >> i) & 1) ? 'C' : 'A';
            bcs.push_back(b);
        }
        const Word w = make_word(bcs);
        std::mt19937_64 rng(m);
        for (int len = 0; len <= m + 5; len++) {   // m + KB + 1 for KB = 4 (shw8: m + k + 1 <= m + 5)
            long n = 1;
            for (int i = 0; i < len; i++) n *= na;
            for (long x = 0; x < n; x++) {
                std::vector<int> t(len);
                long y = x;
                for (int i = 0; i < len; i++) { t[i] = alpha[y % na]; y /= na; }
                run_all(w, {t}, rng, {0}, true);
                counters["targets"]++;
            }
        }
    }
}

// ---- structured random cases
static const char ACGT[] = "ACGT";
static const char IUPAC_BC[] = "NRYKMSWBDHV";

static std::string rand_acgt(std::mt19937_64 &rng, int n) {
    std::string s;
    for (int i = 0; i < n; i++) s += ACGT[rng() % 4];
    return s;
}

// the barcode's letters as text codes (IUPAC letters stay themselves)
static std::vector<int> to_codes(const std::string &s) {
    std::vector<int> t;
    for (char c : s) t.push_back((int)(strchr(kCodes, c) - kCodes));
    return t;
}

static std::vector<int> rand_text(std::mt19937_64 &rng, int n) {
    std::vector<int> t;
    for (int i = 0; i < n; i++) {
        const int r = (int)(rng() % 20);
        t.push_back(r < 16 ? (int)(rng() % 4) : r < 18 ? (int)(4 + rng() % 11) : 15);
    }
    return t;
}

// the barcode with exactly `e` edits, all at its first and last base (substitutions, insertions, deletions)
static std::vector<int> edited(std::mt19937_64 &rng, const std::string &b, int e) {
    std::vector<int> t = to_codes(b);
    for (int i = 0; i < e; i++) {
        const bool front = rng() & 1;
        const int op = (int)(rng() % 3);
        if (t.empty()) { t.push_back((int)(rng() % 4)); continue; }
        const int pos = front ? 0 : (int)t.size() - 1;
        if (op == 0) t[pos] = (t[pos] + 1 + (int)(rng() % 3)) % 4;
        else if (op == 1) t.insert(t.begin() + (front ? 0 : (int)t.size()), (int)(rng() % 4));
        else t.erase(t.begin() + pos);
    }
    return t;
}

static void run_random(int seed) {
    std::mt19937_64 rng(seed);
    FILE *sample = fopen("oracle_sample.txt", "w");
    long nsample = 0;
    for (int iter = 0; iter < 240; iter++) {
        const int m = 1 + iter % 16, nb = 1 + (int)(rng() % 32);
        std::vector<std::string> bcs;
        while ((int)bcs.size() < nb) {
            std::string b;
            const int r = (int)(rng() % 10);
            if (!bcs.empty() && r < 3) {   // 1-2 substitutions from an earlier barcode: ties
                b = bcs[rng() % bcs.size()];
                for (int e = 0, ne = 1 + (int)(rng() % 2); e < ne; e++) b[rng() % m] = ACGT[rng() % 4];
                counters["bc_near"]++;
            } else {
                b = rand_acgt(rng, m);
                if (r == 9) { b[rng() % m] = IUPAC_BC[rng() % 11]; counters["bc_iupac"]++; }
            }
            bcs.push_back(b);
        }
        const Word w = make_word(bcs);
        for (int hi = 0; hi < 12; hi++) {
            const int ne = 1 + (int)(rng() % 3);   // entries of one hit (locations of the primer)
            std::vector<std::vector<int>> targets;
            std::vector<int> offs;
            for (int e = 0; e < ne; e++) {
                const std::string &b = bcs[rng() % nb];
                const int kind = (int)(rng() % 5);
                const int kk = std::min(7, m - 1);
                std::vector<int> t;
                if (kind == 0) {
                    t = edited(rng, b, (int)(rng() % (kk + 2)));
                    auto tail = rand_text(rng, (int)(rng() % 12));
                    t.insert(t.end(), tail.begin(), tail.end());
                    counters["kind_edits"]++;
                } else if (kind == 1) {   // cut by the window end: ncol < m, m - k, m + k, > m + k
                    t = edited(rng, b, (int)(rng() % 3));
                    auto tail = rand_text(rng, 24);
                    t.insert(t.end(), tail.begin(), tail.end());
                    const int k = (int)(rng() % (kk + 1));
                    const int c = (int)(rng() % 4);
                    int n = c == 0 ? (int)(rng() % m) : c == 1 ? m - k : c == 2 ? m + k : m + k + 1 + (int)(rng() % 8);
                    t.resize(std::max(0, n));
                    counters["kind_cut"]++;
                } else if (kind == 2) {   // two barcodes interleaved
                    const std::string &b2 = bcs[rng() % nb];
                    const int ch = 1 + (int)(rng() % 3);
                    std::string s;
                    for (int i = 0; i < m; i += ch) s += b.substr(i, ch) + b2.substr(i, ch);
                    t = to_codes(s);
                    counters["kind_interleaved"]++;
                } else if (kind == 3) {
                    t = rand_text(rng, (int)(rng() % (m + 10)));
                    counters["kind_unrelated"]++;
                } else {   // exact barcode then insert text: distance 0, or a tie when near barcodes exist
                    t = to_codes(b);
                    auto tail = rand_text(rng, (int)(rng() % 10));
                    t.insert(t.end(), tail.begin(), tail.end());
                    counters["kind_exact"]++;
                }
                targets.push_back(t);
                offs.push_back((int)(rng() % 40) - 10);
            }
            run_all(w, targets, rng, offs, false);
            counters["hits"]++;
            // a sample of the reference DP for the suite's oracle
            for (size_t e = 0; e < targets.size(); e++) {
                if (targets[e].empty() || (rng() % 8) != 0) continue;
                const int b = (int)(rng() % nb);
                const std::vector<int> last = dp_last_row(bcs[b], targets[e]);
                int mn = INF, me = -1;
                for (int j = 1; j <= (int)targets[e].size(); j++) {
                    if (last[j] < mn) mn = last[j];
                }
                for (int j = 1; j <= (int)targets[e].size(); j++)
                    if (last[j] == mn) me = j - 1;
                const int k = std::min(7, m - 1);
                std::string ts;
                for (int c : targets[e]) ts += c < 15 ? kCodes[c] : 'X';
                fprintf(sample, "%s %s %d %d %d\n", bcs[b].c_str(), ts.c_str(), k, mn, me);
                nsample++;
            }
        }
    }
    fclose(sample);
    counters["oracle_sample"] = nsample;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "exhaustive")) run_exhaustive(argc >= 3 ? atoi(argv[2]) : 5);
    else if (argc >= 3 && !strcmp(argv[1], "random")) run_random(atoi(argv[2]));
    else {
        fprintf(stderr, "usage: barcode_sim exhaustive [mmax] | random <seed>\n");
        return 2;
    }
    for (const auto &kv : counters) printf("%s %ld\n", kv.first.c_str(), kv.second);
    printf("%ld mismatches\n", mismatches);
    return 0;
}
