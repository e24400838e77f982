// smx_cons_core.h -- the per-pair code of the consensus kernel (smx_cons.hip): NW (global) alignment of one draft, given
// as a Peq table and a byte -> row map, to one read, under smx_pairs_core.h's band, WITH the traceback pairs_pair does
// not keep: the pair's distance and the read's pileup row over the draft.
//
// Forward pass.  pairs_pair's column loop; every active block of every column also leaves its (Pv, Mv) and its bottom
// score in a history, [column][block in band][lane]: block w of column c (1..n) is slot w - F(c) of the column's B slots,
// F(c) the column's first block.  A column runs the blocks that hold a row of [c + dlo, c + dhi], so it has at most
// ((dhi - dlo) >> 6) + 2 of them; B is at least that, or the draft's word count W.
//
// Traceback.  From cell (m, n), one fixed rule:
//   1. diagonal if D[i-1][j-1] + (q[i-1] != t[j-1]) == D[i][j];
//   2. else up if D[i-1][j] + 1 == D[i][j]      (draft base i has no partner: a deletion in the read);
//   3. else left                                  (read base j is an insertion);
// at i = 0 only left is possible, at j = 0 only up.  A cell's value is its block's bottom score less the vertical deltas
// below it; row 0 and column 0 are known (D[0][j] = j, D[i][0] = i); a cell of a block its column did not run counts
// as infinite.
//
// Why the banded walk equals the full-matrix walk.  The walk starts on an exact cell (smx_pairs_core.h: D[m][n] is
// exact when it is <= k) and keeps to exact cells of optimal paths:
//   * a neighbour that passes its equality test has a computed value equal to D[cur] - cost.  Computed band values are
//     never below the truth, and the truth is never below D[cur] - cost (the recurrence at cur).  So the neighbour's
//     value is exact, the full matrix passes the same test, and the neighbour lies on an optimal path.
//   * conversely, a neighbour the full matrix would take lies on an alignment of cost D[m][n] <= k.  It is therefore
//     inside the band -- its block ran in its column -- and by §14's induction its computed value is exact: the banded
//     test passes too.
// Both walks test the neighbours in the same order, so they take the same step from every cell.  The fixed order also
// puts every read's gap in a homopolymer run at the same end of the run, which is what makes column votes meaningful.
//
// The pileup row: m + 1 uint32 words.  Word p < m: bits 0-2 what the read has at draft position p (0-3 = A C G T, 4 = any
// other byte, 5 = deletion), bits 3-10 the length of the read's insertion before position p, clipped to 255, bits 11-22
// the codes of the first SMX_CONS_MAX_INS inserted bytes, 3 bits each, in read order (slots past the length are 0).
// Word m: bits 0-2 are 7, the rest describes the insertion after the last base.  A pair above the limit has no row.
//
// Host/device code like smx_pairs_core.h: the kernel and tests/cpu/cons_sim.cpp run the same functions.
#ifndef SMX_CONS_CORE_H
#define SMX_CONS_CORE_H
#include "smx_pairs_core.h"

#include "smx.h"   // SMX_CONS_MAX_INS, SMX_CONS_VOTE_WORDS (per draft position: sym[6], ins[slot][code < 5])

#define SMX_CONS_DEL 5u
#define SMX_CONS_END 7u

namespace smx {

struct alignas(16) cons_pm { u64 p, m; };   // one block's vertical deltas: one 16-byte store

struct ConsHist {      // pointers already offset to this lane; entry e at [e * MINE_THREADS]
    cons_pm *pm;
    int *s;            // the block's bottom score
    int B;             // slots per column
};

// the code of a read byte: exact bytes, as in clusters ('a' or 'N' are "other")
SMX_HD unsigned cons_code(unsigned char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }

// blocks per column the band of (m, n, k) needs at most: the host sizes B from it
SMX_HD int cons_band_blocks(int m, int n, int k) {
    const int big = m > n ? m : n;
    const int kk = (k < 0 || k > big) ? big : k;
    const int g = m - n, ag = g < 0 ? -g : g;
    if (ag > kk || m == 0 || n == 0) return 0;     // no forward pass
    const int width = ag + 2 * ((kk - ag) >> 1);   // dhi - dlo
    return mine_min((m + 63) >> 6, (width >> 6) + 2);
}

// One pair: the NW distance of the draft (Peq of W words, padded row stride Wp; m = 0: W = 0, never read) and the read
// t[0..n), -1 if it exceeds k (k < 0: no limit); for a pair within the limit row[0..m] receives the pileup row.  t as
// for pairs_pair.  H needs n * H.B entries per lane, H.B >= cons_band_blocks(m, n, k).  WR, st as for pairs_pair.
template <int WR, typename State>
SMX_MINE_HD int cons_pair(State &st, const ConsHist &H, const u64 *peq, const unsigned short *rowmap, int m, int W, int Wp,
                          int k, const unsigned char *t, int n, uint32_t *row) {
    const int big = m > n ? m : n;
    const int kk = (k < 0 || k > big) ? big : k;
    const int g = m - n, ag = g < 0 ? -g : g;
    if (ag > kk) return -1;
    const int e = (kk - ag) >> 1;
    const int dlo = (g < 0 ? g : 0) - e, dhi = (g > 0 ? g : 0) + e;
    const int last = W - 1;
    int dist = big;                                // an empty side: |g| <= kk
    if (m > 0 && n > 0) {                          // ---- forward: pairs_pair's loop, leaving the history
        const int rlast = (m - 1) - 64 * last;
        int L = mine_min(last, dhi >> 6);
        const int wend = WR > 0 ? WR : L + 1;
        constexpr int kUnroll = WR > 0 ? WR : 1;
#pragma unroll kUnroll
        for (int w = 0; w < wend; w++) {
            st.p(w) = ~0ull;
            st.m(w) = 0ull;
            st.s(w) = 64 * (w + 1);
        }
        int sbot = 64 * (L + 1);
        u64 Pl = 0ull, Ml = 0ull;
        const mine_u4 *t16 = reinterpret_cast<const mine_u4 *>(t);
        mine_u4 chunk = mine_u4_zero();
        const int wloop = WR > 0 ? WR : W;
        for (int j = 0; j < n; j++) {              // column j + 1
            if ((j & 15) == 0) chunk = t16[j >> 4];
            const int jj = j & 15;
            const unsigned word = jj < 4 ? chunk.x : jj < 8 ? chunk.y : jj < 12 ? chunk.z : chunk.w;
            const u64 *eqrow = peq + (size_t)rowmap[(word >> (8 * (jj & 3))) & 0xffu] * Wp;
            const int F = j + dlo > 0 ? (j + dlo) >> 6 : 0;
            const int Ln = mine_min(last, (j + dhi) >> 6);
            const bool join = Ln > L;
            L = Ln;
            const size_t col = (size_t)j * H.B - F;            // slot of block w: col + w
            int h = 1;
            bool alive = false;
#pragma unroll kUnroll
            for (int w = 0; w < wloop; w++) {
                if (w > L) break;
                if (w < F) continue;
                if (join && w == L) {
                    st.p(w) = ~0ull;
                    st.m(w) = 0ull;
                    st.s(w) = sbot + 64;
                }
                u64 Pv = st.p(w), Mv = st.m(w);
                h = mine_step(eqrow[w], Pv, Mv, h);
                const int s = st.s(w) + h;
                st.p(w) = Pv;
                st.m(w) = Mv;
                st.s(w) = s;
                H.pm[(col + w) * MINE_THREADS] = cons_pm{Pv, Mv};
                H.s[(col + w) * MINE_THREADS] = s;
                if (s < kk + 64) alive = true;
                if (w == L) { sbot = s; Pl = Pv; Ml = Mv; }
            }
            if (!alive) return -1;
        }
        dist = mine_last_row(Pl, Ml, sbot, rlast);
        if (dist > kk) return -1;
    }
    // ---- traceback
    constexpr int kInf = 0x3fffffff;
    // D[i][c] as the forward pass left it (i, c >= 1)
    auto cell = [&](int i, int c) -> int {
        const int w = (i - 1) >> 6, r = (i - 1) & 63;
        const int F = c - 1 + dlo > 0 ? (c - 1 + dlo) >> 6 : 0, L = mine_min(last, (c - 1 + dhi) >> 6);
        if (w < F || w > L) return kInf;
        const size_t at = ((size_t)(c - 1) * H.B + (w - F)) * MINE_THREADS;
        const cons_pm v = H.pm[at];
        return mine_last_row(v.p, v.m, H.s[at], r);
    };
    int i = m, j = n, cur = dist;
    unsigned sym = SMX_CONS_END, ilen = 0, icodes = 0;         // of word i
    while (i > 0 || j > 0) {
        int step = 2;                                          // 0 = diagonal, 1 = up, 2 = left
        int next = cur - 1;
        unsigned char tc = 0;
        if (j > 0) tc = t[j - 1];
        if (i > 0 && j > 0) {
            const int neq = (int)(~(peq[(size_t)rowmap[tc] * Wp + ((i - 1) >> 6)] >> ((i - 1) & 63)) & 1ull);
            const int dg = i == 1 ? j - 1 : j == 1 ? i - 1 : cell(i - 1, j - 1);
            if (dg + neq == cur) { step = 0; next = dg; }
        }
        if (step == 2 && i > 0) {
            const int up = j == 0 ? i - 1 : i == 1 ? j : cell(i - 1, j);
            if (up + 1 == cur) step = 1;
        }
        if (step == 2) {                                       // read base j sits before draft position i
            ilen++;
            icodes = ((icodes << 3) | cons_code(tc)) & ((1u << (3 * SMX_CONS_MAX_INS)) - 1u);
            j--;
        } else {
            row[i] = sym | ((ilen < 255u ? ilen : 255u) << 3) | (icodes << 11);
            sym = step == 0 ? cons_code(tc) : SMX_CONS_DEL;
            ilen = 0;
            icodes = 0;
            i--;
            if (step == 0) j--;
        }
        cur = next;
    }
    row[0] = sym | ((ilen < 255u ? ilen : 255u) << 3) | (icodes << 11);
    return dist;
}

// What one row word adds to a position's SMX_CONS_VOTE_WORDS counters (sym[6], then ins[slot][code]).  Compares and
// adds over static indices only, so that the vote kernel keeps v in registers.
SMX_HD void cons_vote_word(uint32_t w, uint32_t (&v)[SMX_CONS_VOTE_WORDS]) {
    const unsigned s = w & 7u, len = (w >> 3) & 255u;
#pragma unroll
    for (unsigned c = 0; c < 6; c++) v[c] += s == c;
#pragma unroll
    for (unsigned slot = 0; slot < SMX_CONS_MAX_INS; slot++) {
        const unsigned code = (w >> (11 + 3 * slot)) & 7u;
#pragma unroll
        for (unsigned c = 0; c < 5; c++) v[6 + 5 * slot + c] += (slot < len) & (code == c);
    }
}

}  // namespace smx

#endif  // SMX_CONS_CORE_H
