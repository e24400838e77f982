// smx_inner_core.h -- the per-lane code of the inner scan (smx_inner.hip, smx_inner_scan in include/smx.h): every
// pattern of a panel against the WHOLE read, hits reported for the internal columns.
//
//   * inner_step: the single-word Myers step in search form (row 0 of the DP is 0 in every column), returning the change
//     of the last row's value D(c).
//   * a read's internal columns [margin, n - margin) are cut into pieces of PL columns; one lane owns one (read, piece)
//     unit and G patterns.  It starts `lead` = max(m + k) columns before its piece from the fresh column D[i] = i: an
//     alignment of distance <= k spans at most m + k read columns, so every value <= k inside the piece is exact and
//     every other value stays > k (starting late can only raise a value).  Column 0 of a read IS the fresh column.
//   * InnerTrack follows the runs of consecutive columns with D <= k inside the piece and leaves one record per
//     (unit, pattern): the run count, whether the first run starts on the piece's first column and the last run ends on
//     its last one, the first H runs and the last run.
//   * inner_merge walks the records of one (read, pattern) in piece order, joins runs that cross a piece boundary and
//     writes the outputs; for any piece length they are those of the definition over the whole read.
//
// Host/device code: the kernels and the CPU unit test (tests/cpu/inner_sim.cpp) run the same functions.
#ifndef SMX_INNER_CORE_H
#define SMX_INNER_CORE_H
#include <stddef.h>
#include <stdint.h>

#include "smx_mine_core.h"   // SMX_HD, SMX_MINE_HD, mine_u4

#define INNER_THREADS 256        // lanes (units) per workgroup
#define INNER_MAX_PATTERNS 128
#define INNER_MAX_HITS 8
#define INNER_COUNT_CAP 65536    // the merged hit count stops here (nhit saturates at 255 anyway)

namespace smx {

// piece length for a call whose largest m + k is `lead`: the warm-up costs at most a quarter of the piece
SMX_HD int inner_piece_len(int lead) {
    int pl = 64;
    while (pl < 4 * lead && pl < 512) pl *= 2;
    return pl;
}

// 32-bit words of one (unit, pattern) record: header, last run, first H runs
SMX_HD int inner_rec_words(int H) { return 2 + H; }
// a run inside a piece: the offset of its end column from the piece's first column, and its distance
SMX_HD uint32_t inner_pack_run(int off, int d) { return (uint32_t)off | ((uint32_t)d << 16); }
#define INNER_F_FIRST (1u << 16)   // header: the first run starts on the piece's first column
#define INNER_F_LAST (1u << 17)    // header: the last run ends on the piece's last column

// bit sh of x (one v_bfe_u32 for a 32-bit word on the device)
template <typename W>
SMX_HD int inner_bit(W x, int sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (sizeof(W) == 4) return (int)__builtin_amdgcn_ubfe((unsigned)x, (unsigned)sh, 1u);
#endif
    return (int)((x >> sh) & 1);
}

// One column of pattern (Pv, Mv) with match word Eq; msh = m - 1.  Returns D(c) - D(c - 1) of the last row.
template <typename W>
SMX_HD int inner_step(W Eq, W &Pv, W &Mv, int msh) {
    const W Xv = Eq | Mv;
    const W Xh = (W)((((Eq & Pv) + Pv) ^ Pv) | Eq);
    W Ph = (W)(Mv | ~(Xh | Pv));
    W Mh = (W)(Pv & Xh);
    const int dh = inner_bit<W>(Ph, msh) - inner_bit<W>(Mh, msh);
    Ph = (W)(Ph << 1);
    Mh = (W)(Mh << 1);
    Pv = (W)(Mh | ~(Xv | Ph));
    Mv = (W)(Ph & Xv);
    return dh;
}

struct InnerTrack {
    int rmin;    // distance of the open run, -1: none
    int rend;    // its end: offset of the first column that attains rmin
    int nruns;   // closed runs, | INNER_F_FIRST
};

SMX_HD void inner_track_init(InnerTrack &t) {
    t.rmin = -1;
    t.rend = 0;
    t.nruns = 0;
}

SMX_HD void inner_track_close(InnerTrack &t, int H, uint32_t *rec) {
    const uint32_t run = inner_pack_run(t.rend, t.rmin);
    const int n = t.nruns & 0xffff;
    rec[1] = run;
    if (n < H) rec[2 + n] = run;
    if (n < 0xffff) t.nruns++;
    t.rmin = -1;
}

// column at offset o of the piece, last-row value d; rec = the (unit, pattern) record
SMX_HD void inner_track_col(InnerTrack &t, int d, int k, int o, int H, uint32_t *rec) {
    if (d <= k) {
        if (t.rmin < 0) {
            if (o == 0) t.nruns |= (int)INNER_F_FIRST;
            t.rmin = d;
            t.rend = o;
        } else if (d < t.rmin) {
            t.rmin = d;
            t.rend = o;
        }
    } else if (t.rmin >= 0) {
        inner_track_close(t, H, rec);
    }
}

SMX_HD void inner_track_finish(InnerTrack &t, int H, uint32_t *rec) {
    uint32_t last = 0;
    if (t.rmin >= 0) {
        inner_track_close(t, H, rec);
        last = INNER_F_LAST;
    }
    rec[0] = (uint32_t)t.nruns | last;
}

// One unit: piece `piece` of a read of n bytes that starts at byte roff of b16 (16-byte words; readable up to the
// word that holds the read's last byte), for the G patterns of one pass:
//   peq[code * G + g]  match word of pattern g for read code `code` (16 codes); lut[byte] = code
//   pm / pk / jmap     per pattern: length, threshold (-1 on a padding slot: never a hit) and its index j in the call
//                      (< 0 on a padding slot: no record)
//   rec_unit           the unit's records, pattern j at rec_unit + j * inner_rec_words(H)
template <typename W, int G>
SMX_MINE_HD void inner_scan_piece(const W *peq, const unsigned char *lut, const int *pm, const int *pk, const int *jmap,
                                  const mine_u4 *b16, uint64_t roff, int n, int margin, int PL, int lead, int piece, int H,
                                  uint32_t *rec_unit) {
    const int RW = inner_rec_words(H);
    const int start = margin + piece * PL;
    int end = n - margin;
    if (end - start > PL) end = start + PL;
    const int c0 = start > lead ? start - lead : 0;
    W Pv[G], Mv[G];
    int sc[G], msh[G], kk[G];
    InnerTrack tr[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        Pv[g] = (W)~(W)0;
        Mv[g] = (W)0;
        sc[g] = pm[g];
        msh[g] = pm[g] - 1;
        kk[g] = pk[g];
        inner_track_init(tr[g]);
    }
    mine_u4 chunk = mine_u4_zero();
    bool open = false;   // some pattern has an open run
    for (int c = c0; c < end; c++) {
        const uint64_t pos = roff + (uint64_t)c;
        const int jj = (int)(pos & 15);
        if (jj == 0 || c == c0) chunk = b16[pos >> 4];
        const unsigned word = jj < 4 ? chunk.x : jj < 8 ? chunk.y : jj < 12 ? chunk.z : chunk.w;
        const W *row = peq + (size_t)lut[(word >> (8 * (jj & 3))) & 0xffu] * G;
        bool event = open;
#pragma unroll
        for (int g = 0; g < G; g++) {
            sc[g] += inner_step<W>(row[g], Pv[g], Mv[g], msh[g]);
            event = event || sc[g] <= kk[g];
        }
        // the rare path (a value <= k, or a run that ends) is the only one that touches the trackers and the records:
        // one branch per column for all G patterns
        if (event && c >= start) {
            open = false;
#pragma unroll
            for (int g = 0; g < G; g++) {
                if (sc[g] <= kk[g] || tr[g].rmin >= 0)
                    inner_track_col(tr[g], sc[g], kk[g], c - start, H, rec_unit + (size_t)jmap[g] * RW);
                open = open || tr[g].rmin >= 0;
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++)
        if (jmap[g] >= 0) inner_track_finish(tr[g], H, rec_unit + (size_t)jmap[g] * RW);
}

// One (read, pattern): the records of the read's npieces units (the first is unit u0 of recs, Q patterns per unit) ->
// nhit (one byte), hd / he (H slots each).
SMX_MINE_HD inline void inner_merge(const uint32_t *recs, uint64_t u0, int npieces, int Q, int j, int H, int margin,
                                    int PL, uint8_t *nhit, int8_t *hd, int32_t *he) {
    const int RW = inner_rec_words(H);
    int total = 0, omin = 0, oend = 0;
    bool open = false;
#define INNER_EMIT(d, e)                                   \
    do {                                                   \
        if (total < H) { hd[total] = (int8_t)(d); he[total] = (e); } \
        if (total < INNER_COUNT_CAP) total++;              \
    } while (0)
    for (int p = 0; p < npieces; p++) {
        const uint32_t *rec = recs + ((u0 + (uint64_t)p) * (uint64_t)Q + (uint64_t)j) * (uint64_t)RW;
        const uint32_t h = rec[0];
        const int n = (int)(h & 0xffffu);
        const bool f0 = (h & INNER_F_FIRST) != 0, f1 = (h & INNER_F_LAST) != 0;
        const int base = margin + p * PL;
        if (open && (n == 0 || !f0)) {         // the run that reached the previous piece's last column ends there
            INNER_EMIT(omin, oend);
            open = false;
        }
        if (n == 0) continue;
        const int nstored = n < H ? n : H;
        for (int s = 0; s <= nstored; s++) {
            uint32_t run;
            int i;
            if (s < nstored) {
                run = rec[2 + s];
                i = s;
            } else {
                if (n <= H) break;
                // runs H .. n - 2 are not in the record: the H output slots are full by now, they only count
                total = mine_min(total + (n - H - 1), INNER_COUNT_CAP);
                run = rec[1];
                i = n - 1;
            }
            const int d = (int)(run >> 16), e = base + (int)(run & 0xffffu);
            const bool stays_open = i == n - 1 && f1;
            if (i == 0 && open) {              // f0 holds: this run continues the open one
                if (d < omin) { omin = d; oend = e; }
                if (!stays_open) { INNER_EMIT(omin, oend); open = false; }
            } else if (stays_open) {
                open = true;
                omin = d;
                oend = e;
            } else {
                INNER_EMIT(d, e);
            }
        }
    }
    if (open) INNER_EMIT(omin, oend);
#undef INNER_EMIT
    for (int s = total < H ? total : H; s < H; s++) { hd[s] = -1; he[s] = 0; }
    *nhit = (uint8_t)(total < 255 ? total : 255);
}

}  // namespace smx

#endif  // SMX_INNER_CORE_H
