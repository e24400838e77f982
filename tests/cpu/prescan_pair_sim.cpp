// CPU checks of the primer DP's column bookkeeping (specimux_amd/csrc/smx_prescan_core.h, smx_bitslice_core.h), at the
// shapes where a pairing of text columns or a counter can go wrong.  Built and run by tests/test_prescan_pair_cpu.py
// (g++, no GPU).
//   prescan_pair_sim unit            the single-ripple counter update against the two-ripple one (exhaustive), and both
//                                    forms of transpose32 against the definition out[r] bit q = in[q] bit r
//   prescan_pair_sim dp S MR seed    one tile of reads through the transpose phases and prescan_dp<MR, ...>, every flag word,
//                                    the decode and the match word against a plain O(mn) DP.  Primers of 1, 2, MR - 1 and MR
//                                    nt (inert rows above the pattern; the first and the last row of a column), and one with
//                                    four degenerate-letter sets (NX = 4); reads shorter than the window among them.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "smx_prescan_core.h"

using namespace smx;

static bool eq_iupac(unsigned char p, unsigned char t) {
    static const char *pairs[] = {"YC", "YT", "RA", "RG", "NA", "NC", "NG", "NT", "WA", "WT", "MA", "MC", "SC", "SG",
                                  "KG", "KT", "BC", "BG", "BT", "DA", "DG", "DT", "HA", "HC", "HT", "VA", "VC", "VG"};
    if (p == t) return true;
    for (const char *q : pairs)
        if (q[0] == p && q[1] == t) return true;
    return false;
}
static char comp(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }

// ---- unit checks ---------------------------------------------------------------------------------------------------
// the update the single ripple replaces: an increment ripple, then a decrement ripple
static void two_ripples(unsigned (&g)[5], unsigned inc, unsigned dec) {
    unsigned cy = inc, bw = dec, t;
    for (int i = 0; i < 4; i++) { t = g[i] & cy; g[i] ^= cy; cy = t; }
    g[4] ^= cy;
    for (int i = 0; i < 4; i++) { t = ~g[i] & bw; g[i] ^= bw; bw = t; }
    g[4] ^= bw;
}
static unsigned counter_at(const unsigned (&g)[5], int bit) {
    unsigned v = 0;
    for (int i = 0; i < 5; i++) v |= ((g[i] >> bit) & 1u) << i;
    return v;
}

static long check_counter() {
    long bad = 0, n = 0;
    std::mt19937 rng(12345);
    for (int v = 0; v < 32; v++)
        for (int bit = 0; bit < 32; bit++)
            for (int op = 0; op < 3; op++) {   // the checked position: +1, -1, 0; every other position: random value and update
                unsigned g[5], inc = rng(), dec = rng() & ~inc;
                for (int i = 0; i < 5; i++) g[i] = (rng() & ~(1u << bit)) | (((unsigned)v >> i) & 1u) << bit;
                inc = (inc & ~(1u << bit)) | (op == 0 ? 1u << bit : 0u);
                dec = (dec & ~(1u << bit)) | (op == 1 ? 1u << bit : 0u);
                unsigned a[5], b[5];
                memcpy(a, g, sizeof g); memcpy(b, g, sizeof g);
                two_ripples(a, inc, dec);
                bs_updown5(b[0], b[1], b[2], b[3], b[4], inc, dec);
                const unsigned want = (unsigned)(v + (op == 0) - (op == 1)) & 31u;
                n++;
                if (memcmp(a, b, sizeof a) != 0 || counter_at(b, bit) != want) {
                    if (bad < 10) printf("COUNTER value %d bit %d op %d: %u, expected %u\n", v, bit, op, counter_at(b, bit), want);
                    bad++;
                }
            }
    printf("counter: %ld updates checked, %ld mismatches\n", n, bad);
    return bad;
}

static long check_transpose_one(const unsigned (&in)[32], const char *what, long idx) {
    long bad = 0;
    for (int form = 0; form < 2; form++) {
        unsigned a[32];
        memcpy(a, in, sizeof a);
        if (form) transpose32_fields(a); else transpose32(a);
        for (int r = 0; r < 32; r++)
            for (int q = 0; q < 32; q++)
                if (((a[r] >> q) & 1u) != ((in[q] >> r) & 1u)) {
                    if (bad < 10) printf("TRANSPOSE %s %ld form %d: out[%d] bit %d\n", what, idx, form, r, q);
                    bad++;
                }
    }
    return bad;
}
static long check_transpose() {
    long bad = 0, n = 0;
    unsigned m[32];
    for (int r = 0; r < 32; r++) m[r] = 1u << r;
    bad += check_transpose_one(m, "identity", 0); n++;
    for (int r = 0; r < 32; r++)
        for (int q = 0; q < 32; q++) {
            memset(m, 0, sizeof m);
            m[r] = 1u << q;
            bad += check_transpose_one(m, "single bit", r * 32 + q); n++;
        }
    std::mt19937 rng(777);
    for (int k = 0; k < 200; k++) {
        for (int r = 0; r < 32; r++) m[r] = rng();
        bad += check_transpose_one(m, "random", k); n++;
    }
    printf("transpose32: %ld matrices checked in both forms, %ld wrong bits\n", n, bad);
    return bad;
}

// ---- the DP at pair and chunk boundaries ---------------------------------------------------------------------------
static std::vector<int> reference_scores(const std::string &pat, const std::string &text) {
    const int m = (int)pat.size(), n = (int)text.size();
    std::vector<int> col(m + 1), score(n);
    for (int i = 0; i <= m; i++) col[i] = i;
    for (int j = 0; j < n; j++) {
        int diag = col[0];
        col[0] = 0;
        for (int i = 1; i <= m; i++) {
            const int v = std::min(std::min(col[i] + 1, col[i - 1] + 1),
                                   diag + (eq_iupac((unsigned char)pat[i - 1], (unsigned char)text[j]) ? 0 : 1));
            diag = col[i];
            col[i] = v;
        }
        score[j] = col[m];
    }
    return score;
}

template <int MR>
static long run_dp(int S, unsigned seed) {
    const int CH = S / 16, ppr = 2 * CH;
    std::mt19937 rng(seed);
    auto rnd_base = [&] { return "ACGT"[rng() & 3]; };
    auto rnd_seq = [&](int n) { std::string s(n, 'A'); for (auto &c : s) c = rnd_base(); return s; };
    // primers of 1, 2, MR - 1 and MR nt; the fifth has the four degenerate-letter sets R, Y, K, N (symbols 4 .. 7)
    std::vector<std::string> pats = {rnd_seq(1), rnd_seq(2), rnd_seq(MR - 1), rnd_seq(MR), rnd_seq(MR - 2)};
    {
        std::string &d = pats[4];
        const char deg[4] = {'R', 'Y', 'K', 'N'};
        for (int x = 0; x < 4; x++) { d[1 + 4 * x] = deg[x]; d[MR - 4 - 3 * x] = deg[x]; }
    }
    std::vector<int> lens, ks = {0, 1, (MR - 1) / 4, MR / 4, (MR - 2) / 4};
    std::vector<const char *> pp;
    for (auto &s : pats) { lens.push_back((int)s.size()); pp.push_back(s.c_str()); }
    const int NP = (int)pats.size();
    PreDesc D;
    memset(&D, 0, sizeof(D));
    if (!prescan_build_desc(&D, NP, S, pp.data(), lens.data(), ks.data(), eq_iupac)) { printf("desc failed\n"); return 1; }
    if (D.nsym != PRE_MAXSYM) { printf("expected %d symbols, got %d\n", PRE_MAXSYM, D.nsym); return 1; }
    const int n = PRE_TILE;
    std::vector<unsigned char> win((size_t)n * 2 * S, 0);
    std::vector<std::string> heads(n), tails(n);
    std::vector<int> rlen(n);
    for (int r = 0; r < n; r++) {
        std::string h = rnd_seq(S), t = rnd_seq(S);
        for (int e = 0; e < 2; e++) {   // plant mutated copies, in the orientation the scan sees them
            if (rng() % 4 == 0) continue;
            const std::string &pat = pats[2 + rng() % 3];
            std::string cp;
            for (char c : pat) {
                char b = c;
                if (!strchr("ACGT", c)) { do { b = rnd_base(); } while (!eq_iupac((unsigned char)c, (unsigned char)b)); }
                const unsigned u = rng() % 100;
                if (u < 6) b = rnd_base();
                else if (u < 9) continue;
                else if (u < 12) cp.push_back(rnd_base());
                cp.push_back(b);
            }
            if ((int)cp.size() > S) cp.resize(S);   // (S = 16 with a longer primer: the copy runs off the window)
            int pos = (int)(rng() % (S - cp.size() + 1));
            if (rng() % 4 == 0) pos = S - (int)cp.size();   // flush with the window end: the last pair of the run
            if (rng() % 4 == 0) pos = 0;
            if (e) t.replace(pos, cp.size(), cp);
            else {
                std::string rc(cp.rbegin(), cp.rend());
                for (auto &c : rc) c = comp(c);
                h.replace(pos, cp.size(), rc);
            }
        }
        if (r % 97 == 0) { h.assign(S, 'A'); t.assign(S, 'T'); }
        int L = S + 100;
        if (r % 9 == 0) { L = (int)(rng() % (S + 1)); if (r % 27 == 0) L = S - 1 - (int)(rng() % 3); }   // shorter than the window
        rlen[r] = L;
        if (L < S) { h.resize(L); t.resize(L); }
        heads[r] = h; tails[r] = t;
        memcpy(&win[(size_t)r * 2 * S], h.data(), h.size());
        memcpy(&win[(size_t)r * 2 * S + S], t.data(), t.size());
    }
    std::vector<unsigned> gpl((size_t)CH * 8 * 64 * 4, 0u);
    for (int sub = 0; sub < PRE_G / PRE_SUBG; sub++) {
        std::vector<unsigned> planes((size_t)ppr * PRE_CS + 64, 0u);
        const int r0 = sub * PRE_SUBG * 32;
        for (int q = 0; q < PRE_SUBG * 32 * ppr; q++) {
            const int rs = q / ppr, c = q % ppr, read = r0 + rs;
            unsigned w[4];
            memcpy(w, &win[(size_t)read * 2 * S + 16 * c], 16);
            if (c < CH && rlen[read] < S) prescan_short_head_piece(&win[(size_t)read * 2 * S], c, S, rlen[read], w);
            prescan_store_piece(planes.data(), rs, c, w[0], w[1], w[2], w[3]);
        }
        for (int b = 0; b < PRE_SUBG * ppr; b++) {
            const int g = b / ppr, c = b % ppr;
            unsigned o[32];
            prescan_transpose_block(planes.data(), g, c, CH, o);
            for (int d = 0; d < 32; d++)
                gpl[prescan_plane_word(prescan_block_chunk(c, CH), prescan_block_lane(sub * PRE_SUBG + g, c, CH), d)] = o[d];
        }
    }
    std::vector<unsigned> scratch(PRE_SCRATCH);
    std::vector<unsigned> words((size_t)CH * 32), words0((size_t)CH * 32);
    const int MW = (S + 31) / 32;
    long bad = 0, checked = 0, matched = 0;
    for (int p = 0; p < NP; p++)
        for (int lane = 0; lane < 64; lane++) {
            const int g = lane >> 1, X = lane & 1;
            unsigned mword = 0, unused = 0;
            prescan_dp<MR, PRE_MAXSYM - 4, 1>(gpl.data(), scratch.data(), lane, CH, D, p, words.data(), 32, &mword);
            if (p < 4) {   // the variant without extra symbol rows and without the match word writes the same flag words
                prescan_dp<MR, 0, 0>(gpl.data(), scratch.data(), lane, CH, D, p, words0.data(), 32, &unused);
                if (words0 != words) { if (bad < 10) printf("VARIANT primer %d lane %d: <MR, 0, 0> differs\n", p, lane); bad++; }
            }
            const int m = (int)pats[p].size();
            for (int r = 0; r < 32; r++) {
                const int read = g * 32 + r;
                std::string text;
                if (X) text = tails[read];
                else { text.assign(heads[read].rbegin(), heads[read].rend()); for (auto &c : text) c = comp(c); }
                const std::vector<int> score = reference_scores(pats[p], text);
                const int NV = (int)text.size();
                int run = m;
                bool ok = true;
                for (int j = 0; j < NV; j++) {
                    const bool lt = score[j] < run;
                    if (lt) run = score[j];
                    const bool e = score[j] == run;
                    const unsigned w = words[(size_t)(j >> 4) * 32 + r];
                    if (((w >> (j & 15)) & 1u) != (unsigned)lt || ((w >> (16 + (j & 15))) & 1u) != (unsigned)e) ok = false;
                }
                unsigned mrow[9];
                int jstar = -1, nloc = -1;
                const int best = prescan_decode<0>(words.data() + r, 32, CH, MW, m, ks[p], NV, mrow, &jstar, &nloc);
                if (best != run) ok = false;
                const bool mb = (mword >> r) & 1u;   // the match word: best <= k; a superset for reads shorter than the window
                if (NV == S ? mb != (run <= ks[p]) : (run <= ks[p] && !mb)) ok = false;
                if (run <= ks[p]) {
                    matched++;
                    int ejs = -1, en = 0;
                    for (int j = 0; j < S; j++)
                        if (j < NV && score[j] == run) {
                            if (ejs < 0) ejs = j;
                            en++;
                            if (!((mrow[j >> 5] >> (j & 31)) & 1u)) ok = false;
                        } else if ((mrow[j >> 5] >> (j & 31)) & 1u) ok = false;
                    if (ejs != jstar || en != nloc) ok = false;
                }
                checked++;
                if (!ok) {
                    if (bad < 10) printf("MISMATCH read %d primer %d (m %d) end %d (best %d, expected %d)\n", read, p, m, X, best, run);
                    bad++;
                }
            }
        }
    printf("S=%d MR=%d seed=%u: %ld alignments checked, %ld matched, %ld mismatches\n", S, MR, seed, checked, matched, bad);
    return bad;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "unit")) {
        const long bad = check_counter() + check_transpose();
        printf("unit: %ld mismatches\n", bad);
        return bad ? 1 : 0;
    }
    if (argc > 4 && !strcmp(argv[1], "dp")) {
        const int S = atoi(argv[2]), MR = atoi(argv[3]);
        const unsigned seed = (unsigned)atoi(argv[4]);
        long bad = -1;
        if (S >= 16 && S % 16 == 0) {
            if (MR == 22) bad = run_dp<22>(S, seed);
            else if (MR == 24) bad = run_dp<24>(S, seed);
            else if (MR == 31) bad = run_dp<31>(S, seed);
        }
        if (bad < 0) { printf("usage: dp S MR seed with S a multiple of 16, MR 22, 24 or 31\n"); return 2; }
        return bad ? 1 : 0;
    }
    printf("usage: prescan_pair_sim unit | dp S MR seed\n");
    return 2;
}
