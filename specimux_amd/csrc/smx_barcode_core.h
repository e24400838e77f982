// smx_barcode_core.h -- the bit-sliced barcode scans of the demux kernel's lean mode (phase 3b / 3c of smx_demux_tile.h)
// and the host-side fill of their tables.  Which scan and which padded height M a barcode length runs at is decided at
// the call sites in DemuxTile (phase3b_barcodes, phase3c_summary).
//
// This header is host/device code: the kernel and the CPU unit test (tests/cpu/barcode_sim.cpp) run the same functions;
// on the host the table block and the target codes are plain arrays and a "lane" is one call.  The only device-only
// intrinsic, the scheduling barrier of the padded scans, sits behind bs_sched_barrier().
//
// Table block of one 32-barcode word: unsigned [16 rows][16 codes] (256 words); bit b of block[row * 16 + code] is
// set iff barcode b matches text code `code` at row `row`.  The scans read row * 16 + code for row < M (rows < m for
// the unpadded scan), code 0..15, and target bytes cw[0 .. M + KB) (the unpadded scan: cw[0 .. min(ncol, m + k))).
#ifndef SMX_BARCODE_CORE_H
#define SMX_BARCODE_CORE_H

#include "smx_hd.h"
#include "smx_bitslice_core.h"

namespace smx {

SMX_HD void bs_sched_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);
#endif
}

// Bit-sliced SHW scan: ONE lane aligns up to 32 barcodes (one word of the primer's barcode list) against one
// target at once.  Bit b of every word belongs to barcode b.  Per DP cell (row i = barcode position, column c =
// target position) the unit-cost recurrence on the vertical / horizontal deltas in {-1,0,+1} is
//     Z = Eq | Mh_in | Mv_in                       (the cell's minimum is the diagonal value)
//     Ph_out = Mv_in | ~(Z | Pv_in)   Mh_out = Pv_in & Z      (bottom edge, handed to the next column)
//     Pv_out = Mh_in | ~(Z | Ph_in)   Mv_out = Ph_in & Z      (right edge, handed to the next row)
// with SHW boundaries D[0][j] = j, D[i][0] = i.  D[m][c] is kept as a bit-sliced 5-bit counter; seen[d] collects
// the barcodes whose last-row score equalled d (<= k) at some column: exactly what the per-hit distance-level
// bitmasks of the lean summary need (the lowest non-empty level is the best distance, its bits are the tie set).
// Ukkonen band: an alignment of cost <= k never leaves the cells with |column - row| <= k, so only those are
// computed (banded values D' >= D, and D' == D wherever D <= k -- all that seen[] needs).  No boundary special
// cases are required: a row below the band has never been touched and still holds its initial vertical delta
// (+1), which is what "left neighbour = infinity" means for the cell that enters the band; the top in-band cell
// takes (+1) as horizontal delta from above, like row 0 does.  The tracked score B_c = D'(bottom in-band row, c):
// while the band's bottom edge is still descending (c + k <= m - 1) the bottom cell has no left neighbour and
// B_c = B_(c-1) + (1 - Z); once it sits on the last row, B_c = B_(c-1) + (Ph - Mh) as in the full DP.  B_0 = k.
template <int KL>   // KL = number of distance levels kept (k + 1 <= KL): 4 or 8
SMX_HD void bitsliced_shw(const unsigned *re, const unsigned char *cw, int ncol, int m,
                          int kidx, unsigned (&seen)[KL]) {
    unsigned Pv[16], Mv[16];
#pragma unroll
    for (int i = 0; i < 16; i++) { Pv[i] = ~0u; Mv[i] = 0u; }
    const int b0 = kidx < m ? kidx : m;   // D(bottom row of column 0)
    unsigned s0 = (b0 & 1) ? ~0u : 0u, s1 = (b0 & 2) ? ~0u : 0u, s2 = (b0 & 4) ? ~0u : 0u, s3 = (b0 & 8) ? ~0u : 0u,
             s4 = (b0 & 16) ? ~0u : 0u;
#pragma unroll
    for (int d = 0; d < KL; d++) seen[d] = 0u;
    const int ncols = m + kidx;
    constexpr int rs = 16;   // table block layout [row][code]
    for (int c = 0; c < ncols; c++) {
        const unsigned code = c < ncol ? (unsigned)cw[c] : 15u;   // past the window: code 15 matches nothing
        const unsigned *rc = re + code;
        const int rlo = c - kidx, rhi = (c + kidx < m - 1) ? c + kidx : m - 1;   // in-band rows of this column
        const unsigned rows = (rhi >= 0 ? (2u << rhi) - 1u : 0u) & (rlo > 0 ? ~0u << rlo : ~0u);   // one scalar test per row
        unsigned Ph = ~0u, Mh = 0u, Zb = 0u;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if ((rows >> i) & 1u) {
                const unsigned Eq = rc[i * rs];
                const unsigned Z = Eq | Mh | Mv[i];
                const unsigned nPh = Mv[i] | ~(Z | Pv[i]);
                const unsigned nMh = Pv[i] & Z;
                const unsigned nPv = Mh | ~(Z | Ph);
                const unsigned nMv = Ph & Z;
                Pv[i] = nPv; Mv[i] = nMv; Ph = nPh; Mh = nMh;
                Zb = Z;   // the last executed row's Z (rhi)
            }
        }
        if (c + kidx <= m - 1) {   // bottom edge still descending: +1 unless the diagonal is free; an increment ripple alone
            unsigned cy = ~Zb, t;
            t = s0 & cy; s0 ^= cy; cy = t;
            t = s1 & cy; s1 ^= cy; cy = t;
            t = s2 & cy; s2 ^= cy; cy = t;
            t = s3 & cy; s3 ^= cy; cy = t;
            s4 ^= cy;
        } else bs_updown5(s0, s1, s2, s3, s4, Ph, Mh);   // on the last row: score += horizontal delta of row m (disjoint masks)
        if (c >= m - kidx - 1) {   // the tracked cell is on the last row from here on
            const unsigned live = c < ncol ? ~0u : 0u;
            const unsigned hi = ~(s4 | s3) & live;
#pragma unroll
            for (int d = 0; d < KL; d++)
                if (d <= kidx)
                    seen[d] |= hi & ((d & 1) ? s0 : ~s0) & ((d & 2) ? s1 : ~s1) & ((d & 4) ? s2 : ~s2);
        }
    }
}

// Banded DP with a fixed band half-width KB >= k (a wider band than k is still exact: it contains the k band); the
// 2*KB+1 live rows are kept in a circular register window (row r lives in slot r mod WIN, all slot indices static).
// Every barcode is PADDED to M rows by wildcard rows (Eq = all ones for every text code, also
// past the end of the window): the loop bounds no longer depend on the barcode length, so the whole scan unrolls into
// straight-line code -- static row tests, LDS reads at immediate offsets issued ahead of their use, no scalar branches.
// Exactness: a path that reaches (m, j) continues for free along its diagonal to (M, j + M - m), and every other way
// into row M costs at least as much, so min over the live columns of row M equals min over the live columns of row m;
// the lean summary only ever uses that minimum (the lowest non-empty distance level and its bits).  Column c' of row M
// is live iff c' - (M - m) lies inside the window.  M + KB columns instead of m + k: 19 vs 16 for 13-nt barcodes, at
// less than half the instructions per column.
template <int KB, int M>
SMX_HD void bitsliced_shw_pad(const unsigned *re, const unsigned char *cw, int ncol, int m,
                              int kidx, unsigned (&seen)[KB + 1]) {
    constexpr int WIN = 2 * KB + 1, NC = M + KB;
    static_assert(KB < M && M <= 16, "band / padding out of range");
    unsigned Pw[WIN], Mw[WIN];
#pragma unroll
    for (int i = 0; i < WIN; i++) { Pw[i] = ~0u; Mw[i] = 0u; }
    constexpr int b0 = KB;   // D(bottom in-band row of column 0)
    unsigned s0 = (b0 & 1) ? ~0u : 0u, s1 = (b0 & 2) ? ~0u : 0u, s2 = (b0 & 4) ? ~0u : 0u, s3 = (b0 & 8) ? ~0u : 0u,
             s4 = 0u;
#pragma unroll
    for (int d = 0; d <= KB; d++) seen[d] = 0u;
    constexpr int rs = 16;   // table block layout [row][code]: every Eq read is base + code at an immediate offset
    const int nlive = ncol + (M - m);
#pragma unroll
    for (int c = 0; c < NC; c++) {
        // unconditional read (past the window it hits other LDS bytes, never out of the allocation's reach: rows are
        // followed by >= 32 bytes of other regions) + select: no branch, so the column stays one basic block
        const unsigned raw = (unsigned)cw[c];
        const unsigned code = c < ncol ? raw : 15u;
        const unsigned *rc = re + code;
        Pw[(c + KB) % WIN] = ~0u; Mw[(c + KB) % WIN] = 0u;   // the row entering the band: initial vertical delta
        unsigned Ph = ~0u, Mh = 0u, Zb = 0u;
#pragma unroll
        for (int w = 0; w < WIN; w++) {
            const int row = c - KB + w;
            const int sl = ((row % WIN) + WIN) % WIN;
            if (row >= 0 && row < M) {
                const unsigned Eq = rc[row * rs];
                const unsigned Z = Eq | Mh | Mw[sl];
                const unsigned nPh = Mw[sl] | ~(Z | Pw[sl]);
                const unsigned nMh = Pw[sl] & Z;
                const unsigned nPv = Mh | ~(Z | Ph);
                const unsigned nMv = Ph & Z;
                Pw[sl] = nPv; Mw[sl] = nMv; Ph = nPh; Mh = nMh;
                Zb = Z;
            }
        }
        const bool descending = c + KB <= M - 1;
        if (descending) {   // +1 unless the diagonal is free: an increment ripple alone
            unsigned cy = ~Zb, t;
            t = s0 & cy; s0 ^= cy; cy = t;
            t = s1 & cy; s1 ^= cy; cy = t;
            t = s2 & cy; s2 ^= cy; cy = t;
            t = s3 & cy; s3 ^= cy; cy = t;
            s4 ^= cy;
        } else bs_updown5(s0, s1, s2, s3, s4, Ph, Mh);   // score += Ph - Mh (disjoint masks) in one ripple
        if (c >= M - KB - 1) {   // the tracked cell sits on the last row from here on
            const unsigned live = c < nlive ? ~0u : 0u;
            const unsigned hi = ~(s4 | s3) & live;
#pragma unroll
            for (int d = 0; d <= KB; d++)   // levels above k are computed too (no per-level select); the caller ignores them
                seen[d] |= hi & ((d & 1) ? s0 : ~s0) & ((d & 2) ? s1 : ~s1) & ((d & 4) ? s2 : ~s2);
        }
        bs_sched_barrier();   // keep the live ranges column-sized (otherwise ~130 LDS reads get hoisted and spill)
    }
}

// ------------------------------------------------------------------------------------------------
// The same scan for `--trim tails` (models.py:300-319): besides the distance levels it reports, for this location, the
// minimum level of every barcode (ML[d]) and the last live column at which a barcode selected by `want` sits at its own
// minimum -- the end of the alignment the reference keeps for that barcode (all optimal ends of its best alignment).
// Row M, column c' corresponds to row m, column c' - (M - m): a minimum of row m travels down its diagonal for free.
template <int KB, int M>
SMX_HD void bitsliced_shw_pad_tails(const unsigned *re, const unsigned char *cw, int ncol, int m,
                                    int kidx, const unsigned (&want)[KB + 1], unsigned (&seen)[KB + 1],
                                    unsigned (&ML)[KB + 1], int &tailcol) {
    unsigned Hw[2 * KB + 1][KB + 1];
    constexpr int WIN = 2 * KB + 1, NC = M + KB;
    static_assert(KB < M && M <= 16, "band / padding out of range");
    unsigned Pw[WIN], Mw[WIN];
#pragma unroll
    for (int i = 0; i < WIN; i++) { Pw[i] = ~0u; Mw[i] = 0u; }
    constexpr int b0 = KB;   // D(bottom in-band row of column 0)
    unsigned s0 = (b0 & 1) ? ~0u : 0u, s1 = (b0 & 2) ? ~0u : 0u, s2 = (b0 & 4) ? ~0u : 0u, s3 = (b0 & 8) ? ~0u : 0u,
             s4 = 0u;
#pragma unroll
    for (int d = 0; d <= KB; d++) seen[d] = 0u;
    constexpr int rs = 16;   // table block layout [row][code]: every Eq read is base + code at an immediate offset
    const int nlive = ncol + (M - m);
#pragma unroll
    for (int c = 0; c < NC; c++) {
        // unconditional read (past the window it hits other LDS bytes, never out of the allocation's reach: rows are
        // followed by >= 32 bytes of other regions) + select: no branch, so the column stays one basic block
        const unsigned raw = (unsigned)cw[c];
        const unsigned code = c < ncol ? raw : 15u;
        const unsigned *rc = re + code;
        Pw[(c + KB) % WIN] = ~0u; Mw[(c + KB) % WIN] = 0u;   // the row entering the band: initial vertical delta
        unsigned Ph = ~0u, Mh = 0u, Zb = 0u;
#pragma unroll
        for (int w = 0; w < WIN; w++) {
            const int row = c - KB + w;
            const int sl = ((row % WIN) + WIN) % WIN;
            if (row >= 0 && row < M) {
                const unsigned Eq = rc[row * rs];
                const unsigned Z = Eq | Mh | Mw[sl];
                const unsigned nPh = Mw[sl] | ~(Z | Pw[sl]);
                const unsigned nMh = Pw[sl] & Z;
                const unsigned nPv = Mh | ~(Z | Ph);
                const unsigned nMv = Ph & Z;
                Pw[sl] = nPv; Mw[sl] = nMv; Ph = nPh; Mh = nMh;
                Zb = Z;
            }
        }
        const bool descending = c + KB <= M - 1;
        if (descending) {   // +1 unless the diagonal is free: an increment ripple alone
            unsigned cy = ~Zb, t;
            t = s0 & cy; s0 ^= cy; cy = t;
            t = s1 & cy; s1 ^= cy; cy = t;
            t = s2 & cy; s2 ^= cy; cy = t;
            t = s3 & cy; s3 ^= cy; cy = t;
            s4 ^= cy;
        } else bs_updown5(s0, s1, s2, s3, s4, Ph, Mh);   // score += Ph - Mh (disjoint masks) in one ripple
        if (c >= M - KB - 1) {   // the tracked cell sits on the last row from here on
            const unsigned live = c < nlive ? ~0u : 0u;
            const unsigned hi = ~(s4 | s3) & live;
#pragma unroll
            for (int d = 0; d <= KB; d++) {
                const unsigned hd = hi & ((d & 1) ? s0 : ~s0) & ((d & 2) ? s1 : ~s1) & ((d & 4) ? s2 : ~s2);
                Hw[c - (M - KB - 1)][d] = hd;
                seen[d] |= hd;
            }
        }
        bs_sched_barrier();   // keep the live ranges column-sized (otherwise ~130 LDS reads get hoisted and spill)
    }
    unsigned lower = 0;
#pragma unroll
    for (int d = 0; d <= KB; d++) {
        ML[d] = d <= kidx ? (seen[d] & ~lower) : 0u;
        lower |= seen[d];
    }
    tailcol = -1;
#pragma unroll
    for (int ci = 0; ci < 2 * KB + 1; ci++) {
        unsigned any = 0;
#pragma unroll
        for (int d = 0; d <= KB; d++) any |= Hw[ci][d] & ML[d] & want[d];
        tailcol = any ? (M - KB - 1) + ci - (M - m) : tailcol;   // in columns of the unpadded problem
    }
}

// ------------------------------------------------------------------------------------------------
// Host: add barcode `slot` (0..31 of its word) with IUPAC Peq peq16 (bit i of peq16[code]: row i matches text code
// `code`; code 15 matches nothing) and length m <= 16 to the word's table block.  Rows m..15 are wildcards: all ones
// for every code, 15 included (the padded scans read code 15 past the window and need the free diagonal there too).
inline void bs_table_add(unsigned *block, int slot, const unsigned *peq16, int m) {
    for (int row = 0; row < 16; row++)
        for (int c = 0; c < 16; c++)
            if (row >= m || ((peq16[c] >> row) & 1u)) block[row * 16 + c] |= 1u << slot;
}

}  // namespace smx

#endif  // SMX_BARCODE_CORE_H
