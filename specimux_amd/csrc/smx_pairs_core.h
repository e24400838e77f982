// smx_pairs_core.h -- the per-pair code of the clusters kernel (smx_pairs.hip): NW (global) edit distance of one query,
// given as a Peq table and a byte -> row map, to one target, by the multi-word Myers/Hyyro bit-vector of
// smx_mine_core.h (mine_step, mine_last_row, RegState, GlobalState) under a band that moves down the diagonal
// (DESIGN.md §14).
//
// The band.  With g = m - n and e = (k - |g|) / 2, a cell (row i, column j) can lie on an alignment of cost <= k only
// if its diagonal d = i - j satisfies |d| + |d - g| <= k, i.e. min(0, g) - e <= d <= max(0, g) + e: reaching the cell
// costs at least |d| and finishing from it at least |d - g|.  Column j runs the blocks F..L that hold a row of
// [j + dlo, j + dhi]; both ends only move down.
//   * block F, the first of the column, takes hin = +1.  While F = 0 that is the true top row D[0][j] = j; once upper
//     blocks have been dropped it says "the row above grows by one per column", an upper bound (D[i][j] <= D[i][j-1] + 1).
//   * a block that joins at the bottom starts from the +1-per-row column under the bottom score its neighbour had one
//     column earlier, again an upper bound (D[i+1][j] <= D[i][j] + 1).
//   * a column whose every active block has a bottom score >= k + 64 holds no cell <= k: the pair is over (-1).
//
// Why cells <= k stay exact.  Every value the band computes is the DP recurrence over true values or upper bounds of
// them, so it is never below the true D[i][j].  Take an optimal alignment of cost <= k: every cell on it has
// D[i][j] + |d - g| <= k and D[i][j] >= |d|, so it lies inside the band, and its predecessor on the path does too.
// By induction along the path the predecessor's value is exact, the recurrence offers the path's own cost, and the
// computed value is at most -- hence exactly -- D[i][j].  So D[m][n] comes out exact when it is <= k; when it is
// larger the computed value is larger too and the pair reports -1.  The same argument makes the stop rule sound: a
// path of cost <= k crosses every column in a band cell whose exact value is <= k.
//
// Host/device code like smx_mine_core.h: the kernel and tests/cpu/pairs_sim.cpp run the same function.
#ifndef SMX_PAIRS_CORE_H
#define SMX_PAIRS_CORE_H
#include "smx_mine_core.h"

namespace smx {

// One pair: NW distance of the query (Peq of W words, padded row stride Wp; m = 0: W = 0, never read) and the target
// t[0..n).  Returns -1 if the distance exceeds k (k < 0: no limit); an empty side costs the other side's length and is
// compared with k like any other distance.  t must be 16-byte aligned and readable up to the next multiple of 16 bytes
// past n.  WR > 0: the state of W <= WR words in registers; WR = 0: any W, state in st.
template <int WR, typename State>
SMX_MINE_HD int pairs_pair(State &st, const u64 *peq, const unsigned short *rowmap, int m, int W, int Wp, int k,
                           const unsigned char *t, int n) {
    const int big = m > n ? m : n;
    const int kk = (k < 0 || k > big) ? big : k;   // no distance exceeds max(m, n)
    const int g = m - n, ag = g < 0 ? -g : g;
    if (ag > kk) return -1;                        // the length difference alone costs more than k
    if (m == 0 || n == 0) return big;              // = |g| <= kk
    const int e = (kk - ag) >> 1;
    const int dlo = (g < 0 ? g : 0) - e, dhi = (g > 0 ? g : 0) + e;
    const int last = W - 1, rlast = (m - 1) - 64 * last;
    int L = mine_min(last, dhi >> 6);              // column 1's last block; rows [1 + dlo, 1 + dhi]
    const int wend = WR > 0 ? WR : L + 1;
    constexpr int kUnroll = WR > 0 ? WR : 1;       // the register variants unroll fully (static indices)
#pragma unroll kUnroll
    for (int w = 0; w < wend; w++) {               // column 0: D[i][0] = i
        st.p(w) = ~0ull;
        st.m(w) = 0ull;
        st.s(w) = 64 * (w + 1);
    }
    int sbot = 64 * (L + 1);                       // bottom score of block L, one column back
    u64 Pl = 0ull, Ml = 0ull;                      // block L's vectors in the current column
    const mine_u4 *t16 = reinterpret_cast<const mine_u4 *>(t);
    mine_u4 chunk = mine_u4_zero();
    const int wloop = WR > 0 ? WR : W;
    for (int j = 0; j < n; j++) {                  // column j + 1
        if ((j & 15) == 0) chunk = t16[j >> 4];
        const int jj = j & 15;
        const unsigned word = jj < 4 ? chunk.x : jj < 8 ? chunk.y : jj < 12 ? chunk.z : chunk.w;
        const u64 *eqrow = peq + (size_t)rowmap[(word >> (8 * (jj & 3))) & 0xffu] * Wp;
        const int F = j + dlo > 0 ? (j + dlo) >> 6 : 0;        // block of row max(1, j + 1 + dlo)
        const int Ln = mine_min(last, (j + dhi) >> 6);          // block of row j + 1 + dhi; at most L + 1
        const bool join = Ln > L;
        L = Ln;
        int h = 1;
        bool alive = false;
#pragma unroll kUnroll
        for (int w = 0; w < wloop; w++) {
            if (w > L) break;
            if (w < F) continue;
            if (join && w == L) {                  // the block joins: +1 per row under its neighbour's old bottom
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
            if (s < kk + 64) alive = true;         // the block may hold a cell <= k
            if (w == L) { sbot = s; Pl = Pv; Ml = Mv; }
        }
        if (!alive) return -1;
    }
    // column n: row m has d = g, inside the band, so L = last
    const int v = mine_last_row(Pl, Ml, sbot, rlast);
    return v <= kk ? v : -1;
}

}  // namespace smx

#endif  // SMX_PAIRS_CORE_H
