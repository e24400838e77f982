// CPU check of EVERY distance level of the padded barcode scan (specimux_amd/csrc/smx_barcode_core.h, bitsliced_shw_pad,
// the host/device function the gfx950 demux kernel runs): for every d <= KB, seen[d] must be exactly the barcodes whose
// row-M value equals d at some live column of a plain O(M n) SHW DP over the wildcard-padded barcode.  barcode_sim.cpp
// pins the lowest level (what the lean summary reads); the diagonal automaton relies on the stronger property, and so does
// the tails variant's seen[], checked here against the same sets.  Built and run by tests/test_barcode_levels_cpu.py (g++, no
// GPU; once more with -fsanitize=address,undefined: table blocks are exactly 256 words, target buffers exactly M + KB bytes).
//
//   barcode_levels_sim <seed>
//
// Every instantiation <KB, M> the kernel has x every barcode length m = KB + 1 .. M x every ncol = 0 .. M + KB + 2 x words of
// 1, 31 and 32 barcodes x CASES targets: a barcode of the word with 0 .. KB + 1 edits anywhere, shifted by 0 .. 2 leading
// bases, followed by random text; IUPAC codes and code 15 inside the target; IUPAC letters inside barcodes.
// Prints "<counter> <value>" lines (the Python test bounds them from below) and "<n> mismatches".
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

static const char kCodes[] = "ACGTNRYKMSWBDHV";   // text codes 0..14; 15 matches nothing but a wildcard row
static const int CASES = 6;

static bool iupac_eq(char a, char b) {
    if (a == b) return true;
    static const char *pairs[] = {"YC", "YT", "RA", "RG", "NA", "NC", "NG", "NT", "WA", "WT", "MA", "MC", "SC", "SG",
                                  "KG", "KT", "BC", "BG", "BT", "DA", "DG", "DT", "HA", "HC", "HT", "VA", "VC", "VG"};
    for (const char *p : pairs)
        if ((p[0] == a && p[1] == b) || (p[0] == b && p[1] == a)) return true;
    return false;
}
static bool eq_code(char bc, int code) { return code < 15 && iupac_eq(bc, kCodes[code]); }

static std::map<std::string, long> counters;
static long mismatches = 0;

// row M of the SHW DP (D[0][j] = j, D[i][0] = i) of barcode b padded to M rows by wildcards, over `text`: D[M][j], j = 0..n
static std::vector<int> padded_last_row(const std::string &b, int M, const std::vector<int> &text) {
    const int m = (int)b.size(), n = (int)text.size();
    std::vector<int> prev(M + 1), cur(M + 1), last(n + 1);
    for (int i = 0; i <= M; i++) prev[i] = i;
    last[0] = M;
    for (int j = 1; j <= n; j++) {
        cur[0] = j;
        for (int i = 1; i <= M; i++) {
            const bool eq = i > m || eq_code(b[i - 1], text[j - 1]);   // rows m + 1 .. M: wildcards, code 15 included
            cur[i] = std::min(std::min(prev[i] + 1, cur[i - 1] + 1), prev[i - 1] + (eq ? 0 : 1));
        }
        last[j] = cur[M];
        std::swap(prev, cur);
    }
    return last;
}

static std::string rand_barcode(std::mt19937_64 &rng, int m) {
    std::string s;
    for (int i = 0; i < m; i++) s += "ACGT"[rng() % 4];
    if (rng() % 6 == 0) { s[rng() % m] = "NRYKMSWBDHV"[rng() % 11]; counters["bc_iupac"]++; }
    return s;
}

static int rand_code(std::mt19937_64 &rng) {
    const int r = (int)(rng() % 20);
    return r < 16 ? (int)(rng() % 4) : r < 18 ? (int)(4 + rng() % 11) : 15;
}

template <int KB, int M>
static void run_inst(const char *inst, std::mt19937_64 &rng, bool tails) {
    for (int m = KB + 1; m <= M; m++)
        for (int nbi = 0; nbi < 3; nbi++) {
            const int nb = nbi == 0 ? 1 : nbi == 1 ? 31 : 32;
            std::vector<std::string> bcs;
            while ((int)bcs.size() < nb) {
                if (!bcs.empty() && rng() % 4 == 0) {   // one substitution from an earlier barcode
                    std::string b = bcs[rng() % bcs.size()];
                    b[rng() % m] = "ACGT"[rng() % 4];
                    bcs.push_back(b);
                } else bcs.push_back(rand_barcode(rng, m));
            }
            std::unique_ptr<unsigned[]> blk(new unsigned[256]);
            for (int i = 0; i < 256; i++) blk[i] = 0u;
            for (int b = 0; b < nb; b++) {
                unsigned peq[16];
                for (int c = 0; c < 16; c++) {
                    peq[c] = 0;
                    for (int i = 0; i < m; i++)
                        if (eq_code(bcs[b][i], c)) peq[c] |= 1u << i;
                }
                bs_table_add(blk.get(), b, peq, m);
            }
            counters[std::string("words_") + std::to_string(nb)]++;
            for (int ncol = 0; ncol <= M + KB + 2; ncol++)
                for (int cs = 0; cs < CASES; cs++) {
                    // the target: shift + a barcode of the word with e edits + random text, ncol codes
                    std::vector<int> t;
                    for (int i = 0, sh = (int)(rng() % 4) % 3; i < sh; i++) t.push_back((int)(rng() % 4));
                    const std::string &src = bcs[rng() % nb];
                    std::vector<int> core;
                    for (char ch : src) core.push_back((int)(strchr(kCodes, ch) - kCodes));
                    for (int e = (int)(rng() % (KB + 2)); e > 0; e--) {
                        const int op = (int)(rng() % 3), pos = core.empty() ? 0 : (int)(rng() % core.size());
                        if (op == 0 && !core.empty()) core[pos] = (core[pos] + 1 + (int)(rng() % 3)) % 4;
                        else if (op == 1 || core.empty()) core.insert(core.begin() + pos, (int)(rng() % 4));
                        else core.erase(core.begin() + pos);
                    }
                    t.insert(t.end(), core.begin(), core.end());
                    while ((int)t.size() < ncol) t.push_back(rand_code(rng));
                    t.resize(ncol);
                    if (ncol && rng() % 4 == 0) { t[rng() % ncol] = 15; }
                    if (ncol && rng() % 4 == 0) { t[rng() % ncol] = 4 + (int)(rng() % 11); }
                    bool has15 = false, hasiu = false;
                    for (int c : t) { has15 |= c == 15; hasiu |= c >= 4 && c < 15; }
                    counters["targets_code15"] += has15;
                    counters["targets_iupac"] += hasiu;
                    // the padded problem's text: the window's codes, then code 15 up to the last live column
                    const int nlive = ncol + (M - m);
                    std::vector<int> text = t;
                    text.resize(nlive, 15);
                    unsigned want[KB + 1];
                    for (int d = 0; d <= KB; d++) want[d] = 0u;
                    for (int b = 0; b < nb; b++) {
                        const std::vector<int> last = padded_last_row(bcs[b], M, text);
                        int nlev = 0;
                        for (int d = 0; d <= KB; d++)
                            for (int j = 1; j <= nlive; j++)
                                if (last[j] == d) { want[d] |= 1u << b; nlev++; break; }
                        counters["barcode_on_a_level"] += nlev >= 1;
                        counters["barcode_on_two_levels"] += nlev >= 2;
                        counters["barcode_on_no_level"] += nlev == 0;
                    }
                    // exactly M + KB bytes, junk behind the window
                    std::unique_ptr<unsigned char[]> buf(new unsigned char[M + KB]);
                    for (int i = 0; i < M + KB; i++) buf[i] = i < ncol ? (unsigned char)t[i] : (unsigned char)(rng() & 0xFF);
                    const int kidx = (int)(rng() % (KB + 1));
                    unsigned seen[KB + 1];
                    if (!tails) bitsliced_shw_pad<KB, M>(blk.get(), buf.get(), ncol, m, kidx, seen);
                    else {
                        unsigned w[KB + 1], ML[KB + 1];
                        for (int d = 0; d <= KB; d++) w[d] = ~0u;
                        int tc = 0;
                        bitsliced_shw_pad_tails<KB, M>(blk.get(), buf.get(), ncol, m, kidx, w, seen, ML, tc);
                    }
                    for (int d = 0; d <= KB; d++) {
                        if (seen[d] != want[d] && ++mismatches <= 20)
                            printf("MISMATCH %s m=%d nb=%d ncol=%d kidx=%d level %d: %08x vs dp %08x\n", inst, m, nb, ncol,
                                   kidx, d, seen[d], want[d]);
                        if (want[d]) counters[std::string("level_") + std::to_string(d) + "_nonempty"]++;
                    }
                    counters[std::string("calls_") + inst]++;
                    counters[std::string("ncol_") + std::to_string(ncol)]++;
                    if (ncol > M + KB) counters["ncol_past_scan"]++;
                    if (ncol < m) counters["ncol_inside_barcode"]++;
                }
        }
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: barcode_levels_sim <seed>\n");
        return 2;
    }
    std::mt19937_64 rng(atoi(argv[1]));
    run_inst<3, 8>("pad3_8", rng, false);
    run_inst<3, 12>("pad3_12", rng, false);
    run_inst<3, 13>("pad3_13", rng, false);
    run_inst<3, 16>("pad3_16", rng, false);
    run_inst<4, 13>("pad4_13", rng, false);
    run_inst<4, 16>("pad4_16", rng, false);
    run_inst<3, 8>("tails3_8", rng, true);
    run_inst<3, 12>("tails3_12", rng, true);
    run_inst<3, 13>("tails3_13", rng, true);
    run_inst<3, 16>("tails3_16", rng, true);
    for (const auto &kv : counters) printf("%s %ld\n", kv.first.c_str(), kv.second);
    printf("%ld mismatches\n", mismatches);
    return 0;
}
