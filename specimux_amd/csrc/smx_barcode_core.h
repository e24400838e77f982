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

// Device: the value becomes opaque to the optimiser here (no instruction is emitted).  The automaton's states cross a
// column boundary through it: without it the OR trees of several columns are reassociated into one, the early columns' Eq
// words stay live to the end of the scan and spill.
SMX_HD void bs_pin(unsigned &x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(x));
#else
    (void)x;
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

// The padded scan: a bit-sliced diagonal automaton over thresholded states, not a delta-encoded DP.
// Every barcode is PADDED to M rows by wildcard rows (Eq = all ones for every text code, also past the end of the
// window): the loop bounds no longer depend on the barcode length, so the whole scan unrolls into straight-line code --
// static row tests, LDS reads at immediate offsets issued ahead of their use, no scalar branches.  A path that reaches
// (m, j) continues for free along its diagonal to (M, j + M - m), and every other way into row M costs at least as much,
// so min over the live columns of row M equals min over the live columns of row m.  Column c' of row M is live iff
// c' - (M - m) lies inside the window (nlive = ncol + (M - m)).  M + KB columns instead of m + k.
//
// States.  The consumers (phase3b_barcodes ORs the levels into dmask, phase3c_summary reads the lowest) need one fact
// per barcode and level: was D[M][col] == d <= KB at some live column.  That is a thresholded quantity, so the scan
// keeps the booleans A_d(row, col) <=> D[row][col] <= d for d = 0..KB directly, with neither deltas nor a score counter.
// D[row][col] >= |row - col|, hence level d has at most 2d + 1 states per column that can be set, on the diagonals
// delta = row - col in [-d, d]: (KB + 1)^2 words in all, kept per (level, diagonal) in registers at static indices.
//
// Recurrence.  Consuming text position c (col = c -> c + 1), Eq = re[(row - 1) * 16 + code], row = c + 1 + delta:
//     new(d, delta) = (old(d, delta) & Eq)        diagonal step, match
//                   |  old(d-1, delta)            substitution
//                   |  old(d-1, delta+1)          text position skipped     (same row, column c)
//                   |  new(d-1, delta-1)          barcode position skipped  (row - 1, column c + 1: the NEW lower level)
// Terms whose diagonal lies outside [-(d-1), d-1] are absent; a state with row < 0 or row > M is 0; row 0 is the constant
// (c + 1 <= d), all ones wherever it is inside the level's diagonals; column 0 starts as A_d(delta, 0) = (0 <= delta).
// The Eq reads of a column are the rows row - 1 in [c - KB, c + KB] and [0, M), shared by all levels.  Levels are
// updated in ascending order and the old level d - 1 is held in one level's worth of temporaries while level d is made.
//
// Levels.  After column c the last row sits on diagonal delta = M - (c + 1); while |delta| <= KB, for d = |delta|..KB
//     seen[d] |= live & A_d(M) & ~A_(d-1)(M)      (A_(d-1) absent, i.e. 0, when d - 1 < |delta|;  live = c < nlive)
// which is exactly the barcodes whose row-M score is d at that column.  All levels d <= KB are exact (kidx is not needed;
// the caller ignores levels above k).  This is bit for bit what the banded delta DP of bitsliced_shw_pad_tails collects:
// its banded values satisfy D' >= D and D' == D wherever D <= KB, hence {D' == d} == {D == d} for every d <= KB.
template <int KB, int M>
SMX_HD void bitsliced_shw_pad(const unsigned *re, const unsigned char *cw, int ncol, int m,
                              int kidx, unsigned (&seen)[KB + 1]) {
    constexpr int WIN = 2 * KB + 1, NC = M + KB;
    static_assert(KB < M && M <= 16, "band / padding out of range");
    (void)kidx;
    unsigned A[KB + 1][WIN];   // A[d][KB + delta], |delta| <= d
#pragma unroll
    for (int d = 0; d <= KB; d++)
#pragma unroll
        for (int w = 0; w < WIN; w++) A[d][w] = w >= KB ? ~0u : 0u;   // column 0: D[delta][0] = delta <= d
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
        unsigned Eq[WIN];   // Eq[KB + delta]: row - 1 = c + delta
#pragma unroll
        for (int w = 0; w < WIN; w++) {
            const int r1 = c - KB + w;
            Eq[w] = (r1 >= 0 && r1 < M) ? rc[r1 * rs] : 0u;
        }
        unsigned lo[WIN];   // the OLD level d - 1 while level d is updated
#pragma unroll
        for (int w = 0; w < WIN; w++) lo[w] = 0u;
#pragma unroll
        for (int d = 0; d <= KB; d++) {
            unsigned od[WIN];
#pragma unroll
            for (int w = 0; w < WIN; w++) od[w] = A[d][w];
#pragma unroll
            for (int w = KB - d; w <= KB + d; w++) {   // ascending diagonals: new(d-1, delta-1) is already in A[d - 1]
                const int row = c + 1 + (w - KB);
                unsigned v;
                if (row < 0 || row > M) v = 0u;
                else if (row == 0) v = ~0u;
                else {
                    const int dl = d - 1, ad = w - KB < 0 ? KB - w : w - KB;   // |delta|
                    v = od[w] & Eq[w];
                    if (ad <= dl) v |= lo[w];
                    unsigned v2 = 0u;
                    if (w + 1 - KB <= dl && w + 1 - KB >= -dl) v2 |= lo[w + 1];
                    if (w - 1 - KB <= dl && w - 1 - KB >= -dl) v2 |= A[d - 1][w - 1];
                    v |= v2;
                    bs_pin(v);
                }
                A[d][w] = v;
            }
#pragma unroll
            for (int w = 0; w < WIN; w++) lo[w] = od[w];
        }
        const int dM = M - (c + 1), adM = dM < 0 ? -dM : dM;
        if (adM <= KB) {   // the last row is inside the widest level's diagonals from here on
            const unsigned live = c < nlive ? ~0u : 0u;
#pragma unroll
            for (int d = 0; d <= KB; d++)
                if (d >= adM) seen[d] |= live & A[d][KB + dM] & ~(d - 1 >= adM ? A[d - 1][KB + dM] : 0u);
        }
        bs_sched_barrier();   // keep the live ranges column-sized: the Eq reads are not hoisted across columns
    }
}

// ------------------------------------------------------------------------------------------------
// The padded scan for `--trim tails` (models.py:300-319): besides the distance levels it reports, for this location, the
// minimum level of every barcode (ML[d]) and the last live column at which a barcode selected by `want` sits at its own
// minimum -- the end of the alignment the reference keeps for that barcode (all optimal ends of its best alignment).
// Row M, column c' corresponds to row m, column c' - (M - m): a minimum of row m travels down its diagonal for free.
// This one stays on the delta-encoded DP of bitsliced_shw (the recurrence above it), banded with a fixed half-width
// KB >= k (a wider band than k is still exact: it contains the k band); the 2*KB+1 live rows are kept in a circular
// register window (row r lives in slot r mod WIN, all slot indices static), the score of the band's bottom cell in the
// 5-bit counter.  Same padding, same reads and same seen[] as bitsliced_shw_pad (the CPU simulation holds the two
// recurrences against each other on every level d <= KB).
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
