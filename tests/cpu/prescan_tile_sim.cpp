// CPU simulation of the primer prescan on tile codes (specimux_amd/csrc/smx_prescan_core.h: tilecodes_word, prescan_stage_code,
// prescan_copy_codes, prescan_dp with TS = 1): the phases of the tile-codes kernel and the DP with lanes as loop indices and
// LDS as an array, against (a) the planes path (prescan_store_piece, prescan_transpose_block, prescan_dp with TS = 0, the
// row-major codes2) and (b) a plain O(mn) DP per (read, primer, end).  Every flag word, the match word, the flag byte and the
// consumer's decode must agree.  Built and run by tests/test_prescan_tile_cpu.py (g++, no GPU).
//   usage: prescan_tile_sim S n_reads seed
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
        if ((q[0] == p && q[1] == t) || (q[1] == p && q[0] == t)) return true;
    return false;
}

static char comp(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }

// scalar reference: HW alignment, the score of every column
static std::vector<int> reference_scores(const std::string &pat, const std::string &text) {
    const int m = (int)pat.size(), n = (int)text.size();
    std::vector<int> col(m + 1), score(n);
    for (int i = 0; i <= m; i++) col[i] = i;
    for (int j = 0; j < n; j++) {
        int diag = col[0];
        col[0] = 0;
        for (int i = 1; i <= m; i++) {
            int v = std::min(std::min(col[i] + 1, col[i - 1] + 1), diag + (eq_iupac((unsigned char)pat[i - 1], (unsigned char)text[j]) ? 0 : 1));
            diag = col[i];
            col[i] = v;
        }
        score[j] = col[m];
    }
    return score;
}

// one DP call of the row count MR, text source TS; NX = 4 for the primer with degenerate letters, else 0
static void run_dp(int MR, bool degenerate, int TS, const unsigned *text, unsigned *scratch, int lane, int CH, const PreDesc &D, int p,
                   unsigned *words, unsigned *mword) {
#define CALL(MRV, NXV, TSV) prescan_dp<MRV, NXV, 1, TSV>(text, scratch, lane, CH, D, p, words, 32, mword)
#define ROWS(MRV) \
    if (MR == MRV) { if (degenerate) { if (TS) CALL(MRV, PRE_MAXSYM - 4, 1); else CALL(MRV, PRE_MAXSYM - 4, 0); } \
                     else { if (TS) CALL(MRV, 0, 1); else CALL(MRV, 0, 0); } }
    ROWS(22) ROWS(24) ROWS(31)
#undef ROWS
#undef CALL
}

int main(int argc, char **argv) {
    const int S = argc > 1 ? atoi(argv[1]) : 80;
    const int n = argc > 2 ? atoi(argv[2]) : 1025;
    const unsigned seed = argc > 3 ? (unsigned)atoi(argv[3]) : 1;
    if (S < 16 || S % 16 || n < 1) { printf("bad arguments\n"); return 2; }
    const int CH = S / 16, ppr = 2 * CH, MW = (S + 31) / 32;
    const int ntiles = (n + PRE_TILE - 1) / PRE_TILE, npad = ntiles * PRE_TILE;
    std::mt19937 rng(seed);
    auto rnd_base = [&] { return "ACGT"[rng() & 3]; };
    long bad = 0;
    auto fail = [&](const char *fmt, auto... a) { if (bad < 10) { printf(fmt, a...); printf("\n"); } bad++; };

    // ---- the address function: every (read, end, chunk) of the padded batch has a word of its own inside the buffer
    {
        std::vector<unsigned char> seen((size_t)npad * ppr, 0);
        for (int read = 0; read < npad; read++)
            for (int X = 0; X < 2; X++)
                for (int c = 0; c < CH; c++) {
                    const size_t at = tilecodes_word((size_t)read, CH, X, c);
                    if (at >= seen.size()) { fail("ADDRESS read %d end %d chunk %d: word %zu outside %zu", read, X, c, at, seen.size()); continue; }
                    if (seen[at]) fail("ADDRESS read %d end %d chunk %d: word %zu taken twice", read, X, c, at);
                    seen[at] = 1;
                }
        // a DP lane's 32 dwords and a demux tile's runs are contiguous
        if (tilecodes_word(33, CH, 1, 0) != tilecodes_word(32, CH, 1, 0) + 1) fail("ADDRESS not contiguous in the read");
    }

    // ---- patterns: 1, 2, MR - 1 and MR nt for the three row counts; index 1 has four degenerate letter sets (N, Y, K, R)
    const std::string p31 = "ACGTTGCATGCCATGACTGACTAGCTAGCAT";
    std::vector<std::string> pats = {p31.substr(0, 22), "ACGTNACGTYACGKARCA", "G", "CA", p31.substr(3, 21), p31.substr(1, 23),
                                     p31.substr(2, 24), p31.substr(0, 30), p31};
    std::vector<int> lens, ks;
    std::vector<const char *> pp;
    for (auto &s : pats) { lens.push_back((int)s.size()); ks.push_back((int)s.size() / 3); pp.push_back(s.c_str()); }
    const int NP = (int)pats.size();
    PreDesc D;
    memset(&D, 0, sizeof(D));
    if (!prescan_build_desc(&D, NP, S, pp.data(), lens.data(), ks.data(), eq_iupac)) { printf("desc failed\n"); return 2; }
    if (D.nsym != 8) { printf("expected four degenerate letter sets, nsym = %d\n", D.nsym); return 2; }

    // ---- reads: windows [read][2 * S] ASCII (head | tail); lengths 0, 1, S / 2, S - 1, S, 2 S among longer ones
    std::vector<unsigned char> win((size_t)npad * 2 * S, 0);
    std::vector<std::string> heads(n), tails(n);
    std::vector<int> rlen(npad, 0), dirty(n, 0);
    const int special[6] = {0, 1, S / 2, S - 1, S, 2 * S};
    for (int r = 0; r < n; r++) {
        std::string h(S, 'A'), t(S, 'A');
        for (auto &c : h) c = rnd_base();
        for (auto &c : t) c = rnd_base();
        for (int e = 0; e < 2; e++) {   // plant mutated copies in the orientation the scan sees them
            if (rng() % 4 == 0) continue;
            const std::string &pat = pats[rng() % NP];
            std::string cp;
            for (char c : pat) {
                char b = c;
                if (!strchr("ACGT", c)) { do { b = rnd_base(); } while (!eq_iupac((unsigned char)c, (unsigned char)b)); }
                unsigned u = rng() % 100;
                if (u < 6) b = rnd_base();
                else if (u < 9) continue;
                else if (u < 12) cp.push_back(rnd_base());
                cp.push_back(b);
            }
            if ((int)cp.size() >= S) continue;
            int pos = (int)(rng() % (S - cp.size() + 1));
            if (rng() % 8 == 0) pos = S - (int)cp.size();
            if (rng() % 8 == 0) pos = 0;
            if (e) t.replace(pos, cp.size(), cp);
            else {
                std::string rc(cp.rbegin(), cp.rend());
                for (auto &c : rc) c = comp(c);
                h.replace(pos, cp.size(), rc);
            }
        }
        if (r % 97 == 5) { h.assign(S, 'A'); t.assign(S, 'T'); }   // low complexity: many optimal ends
        int L = S + 100;
        if (r % 5 == 0 || r == n - 1) L = special[(r / 5) % 6];
        rlen[r] = L;
        if (L < S) { h.resize(L); t.resize(L); }
        heads[r] = h; tails[r] = t;
        memcpy(&win[(size_t)r * 2 * S], h.data(), h.size());
        memcpy(&win[(size_t)r * 2 * S + S], t.data(), t.size());
    }
    // a window holding N, a window holding lower case (the flag byte must say so; such reads' codes are not consumed)
    for (int r = 3; r < n; r += 29) {
        const int Lw = std::min(rlen[r], S);
        if (Lw < 1) continue;
        const int pos = (int)(rng() % (unsigned)Lw);
        unsigned char &ch = win[(size_t)r * 2 * S + ((r & 1) ? S : 0) + pos];
        ch = ((r / 29) & 1) ? (unsigned char)(ch | 0x20) : (unsigned char)'N';
        dirty[r] = 1;
    }

    // ---- the planes path: transpose kernel phases per sub-tile -> planes, row-major codes2, flag bytes
    std::vector<unsigned> gpl((size_t)ntiles * CH * 8 * 64 * 4, 0u), codes2((size_t)npad * ppr, 0u);
    std::vector<unsigned char> naflag(npad, 0), naflag_t(npad, 0);
    const int SUBR = PRE_SUBG * 32, nsub = ntiles * (PRE_G / PRE_SUBG);
    for (int sub = 0; sub < nsub; sub++) {
        std::vector<unsigned> planes((size_t)ppr * PRE_CS + 64, 0u);
        const int r0 = sub * SUBR;
        for (int q = 0; q < SUBR * ppr; q++) {
            const int rs = q / ppr, c = q % ppr, read = r0 + rs;
            unsigned w[4] = {0, 0, 0, 0};
            if (read < n) memcpy(w, &win[(size_t)read * 2 * S + 16 * c], 16);
            if (read < n && (acgt_mismatch(w[0]) | acgt_mismatch(w[1]) | acgt_mismatch(w[2]) | acgt_mismatch(w[3]))) naflag[read] = 1;
            if (read < n && c < CH && rlen[read] < S) prescan_short_head_piece(&win[(size_t)read * 2 * S], c, S, rlen[read], w);
            const unsigned z = prescan_store_piece(planes.data(), rs, c, w[0], w[1], w[2], w[3]);
            int end, chunk;
            const unsigned zz = codes2_from_piece(z, c, CH, &end, &chunk);
            codes2[codes2_word((size_t)read, CH, end, chunk)] = zz;
        }
        for (int b = 0; b < PRE_SUBG * ppr; b++) {
            const int g = b / ppr, c = b % ppr;
            unsigned o[32];
            prescan_transpose_block(planes.data(), g, c, CH, o);
            unsigned *tile = gpl.data() + (size_t)(sub / 4) * CH * 8 * 64 * 4;
            for (int d = 0; d < 32; d++)
                tile[prescan_plane_word(prescan_block_chunk(c, CH), prescan_block_lane((sub & 3) * PRE_SUBG + g, c, CH), d)] = o[d];
        }
    }
    for (int r = 0; r < n; r++) if (rlen[r] < S) naflag[r] = 1;

    // ---- the tile-codes kernel, phase by phase as the device runs it: lane tid takes pieces tid + u * 256 (phase 1), its own
    // read (phase 1b), items tid + u * 256 of the copy-out
    std::vector<unsigned> tcodes((size_t)npad * ppr, 0xDEADBEEFu);
    for (int sub = 0; sub < nsub; sub++) {
        std::vector<unsigned> stage((size_t)ppr * PRE_TS, 0xDEADBEEFu), flagL(SUBR, 0u);
        const int r0 = sub * SUBR;
        for (int u = 0; u < ppr; u++)
            for (int tid = 0; tid < SUBR; tid++) {
                const int q = tid + u * SUBR, rs = q / ppr, c = q % ppr, read = r0 + rs;
                unsigned w[4] = {0, 0, 0, 0};
                if (read < n) memcpy(w, &win[(size_t)read * 2 * S + 16 * c], 16);
                if (acgt_mismatch(w[0]) | acgt_mismatch(w[1]) | acgt_mismatch(w[2]) | acgt_mismatch(w[3])) flagL[rs] = 1u;
                prescan_stage_code(stage.data(), rs, c, CH, w[0], w[1], w[2], w[3]);
            }
        for (int tid = 0; tid < SUBR; tid++) {
            const int read = r0 + tid;
            if (read >= n) continue;
            naflag_t[read] = (unsigned char)(flagL[tid] != 0u || rlen[read] < S);
            if (rlen[read] < S)
                for (int c = 0; c < CH; c++) {
                    unsigned w[4];
                    prescan_short_head_piece(&win[(size_t)read * 2 * S], c, S, rlen[read], w);
                    prescan_stage_code(stage.data(), tid, c, CH, w[0], w[1], w[2], w[3]);
                }
        }
        unsigned *dst = tcodes.data() + tilecodes_word((size_t)r0, CH, 0, 0);
        for (int i = 0; i < ppr * (SUBR / 4); i++) prescan_copy_codes(stage.data(), dst, i);
    }
    // same dwords in both layouts (all reads of the padded batch: the DP reads whole tiles), same flag bytes, expected flags
    for (int read = 0; read < npad; read++)
        for (int X = 0; X < 2; X++)
            for (int c = 0; c < CH; c++)
                if (tcodes[tilecodes_word((size_t)read, CH, X, c)] != codes2[codes2_word((size_t)read, CH, X, c)])
                    fail("CODES read %d end %d chunk %d: tile codes %08x, codes2 %08x", read, X, c,
                         tcodes[tilecodes_word((size_t)read, CH, X, c)], codes2[codes2_word((size_t)read, CH, X, c)]);
    for (int read = 0; read < n; read++) {
        const bool expect = dirty[read] || rlen[read] < S;
        if ((naflag_t[read] != 0) != expect || naflag_t[read] != naflag[read])
            fail("FLAG read %d: tile codes %d, planes %d, expected %d", read, naflag_t[read], naflag[read], (int)expect);
    }

    // ---- the DP on both text sources, and against the plain DP
    struct Run { int p, MR; };
    std::vector<Run> runs;
    for (int p = 0; p < NP; p++) {
        const int m = lens[p];
        for (int MR : {22, 24, 31})
            if (m <= 2 ? true : (m == MR || m == MR - 1) || (p < 2 && MR == 22)) runs.push_back({p, MR});
    }
    std::vector<unsigned> scratch(PRE_SCRATCH), wp((size_t)CH * 32), wt((size_t)CH * 32);
    long checked = 0, matched = 0;
    for (int tile = 0; tile < ntiles; tile++)
        for (const Run &rn : runs)
            for (int lane = 0; lane < 64; lane++) {
                const int p = rn.p, g = lane >> 1, X = lane & 1;
                if (tile * PRE_TILE + g * 32 >= n) continue;   // (a group of padding only: nothing consumes it)
                unsigned mp = 0, mt = 0;
                run_dp(rn.MR, p == 1, 0, gpl.data() + (size_t)tile * CH * 2048, scratch.data(), lane, CH, D, p, wp.data(), &mp);
                run_dp(rn.MR, p == 1, 1, tcodes.data() + (size_t)tile * CH * 2048, scratch.data(), lane, CH, D, p, wt.data(), &mt);
                if (mp != mt) fail("MATCH WORD tile %d primer %d rows %d lane %d: %08x, planes %08x", tile, p, rn.MR, lane, mt, mp);
                for (size_t i = 0; i < wp.size(); i++)
                    if (wp[i] != wt[i]) { fail("FLAG WORD tile %d primer %d rows %d lane %d word %zu", tile, p, rn.MR, lane, i); break; }
                for (int r = 0; r < 32; r++) {
                    const int read = tile * PRE_TILE + g * 32 + r;
                    if (read >= n || dirty[read]) continue;
                    std::string text;
                    if (X) text = tails[read];
                    else { text.assign(heads[read].rbegin(), heads[read].rend()); for (auto &c : text) c = comp(c); }
                    const std::vector<int> score = reference_scores(pats[p], text);
                    const int NV = (int)text.size(), m = lens[p];
                    int run = m;
                    bool ok = true;
                    for (int j = 0; j < NV; j++) {
                        const bool lt = score[j] < run;
                        if (lt) run = score[j];
                        const bool e = score[j] == run;
                        const unsigned w = wt[(size_t)(j >> 4) * 32 + r];
                        if (((w >> (j & 15)) & 1u) != (unsigned)lt || ((w >> (16 + (j & 15))) & 1u) != (unsigned)e) ok = false;
                    }
                    unsigned mrow[9];
                    int jstar = -1, nloc = -1;
                    const int best = CH == 5 ? prescan_decode<5>(wt.data() + r, 32, CH, MW, m, ks[p], NV, mrow, &jstar, &nloc)
                                             : prescan_decode<0>(wt.data() + r, 32, CH, MW, m, ks[p], NV, mrow, &jstar, &nloc);
                    if (best != run) ok = false;
                    const bool mb = (mt >> r) & 1u;
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
                    if (!ok) fail("MISMATCH read %d (length %d) primer %d rows %d end %d (best %d, expected %d)", read, rlen[read], p, rn.MR, X, best, run);
                }
            }
    printf("S=%d n=%d seed=%u: %zu DP runs per lane, %ld alignments checked, %ld matched, %ld mismatches\n", S, n, seed, runs.size(), checked,
           matched, bad);
    return bad ? 1 : 0;
}
