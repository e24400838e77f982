// smx_flank_core.h -- the per-hit and per-key logic of the barcode survey (specimux-barcodes), host/device.
//
// flank_of_hit(): one (read, primer, end) hit record of the demux kernel's dump + the read's end windows -> what sits
// where the barcode should be (the "flank": the bases behind the primer's first optimal end, the prefix of the string
// match_one_end searches for barcode_rc), as one of five ways out and, for a counted hit, a 64-bit key (layout:
// include/smx.h, "Barcode survey").  flank_shw(): the prefix (SHW) edit distance of one candidate barcode to the flank
// a key holds; flank_take(): a key's running best candidate.  The (key, count) table is smx_stats_core.h's.
// Shared by smx_flank.hip and tests/cpu/flank_sim.cpp, which runs this code without a GPU.
#ifndef SMX_FLANK_CORE_H
#define SMX_FLANK_CORE_H
#include <stdint.h>
#include "smx.h"
#include "smx_stats_core.h"

namespace smx {

// shape of the count kernel's on-chip combine (smx_flank.hip); the CPU simulation walks the hits in the same chunks
#define FLANK_THREADS 256
#ifndef FLANK_LCAP               // (the simulation is also built with a tiny table, to drive keys past it)
// A workgroup of a 765k-read launch sees about 3 000 counted hits (1.5 M over 2 workgroups on each of 256 CUs).  A key
// holds W = Lb + k bases, so even an error-free barcode comes with 4^k = 64 different tails behind it: the mass that sits
// on a few hundred exact barcodes is spread over 64 keys each (c2: 56 barcodes, some 3 600 popular keys holding a third
// of the hits), and the rest is a tail of singletons, 650 distinct flanks per 1 000 hits.  What the LDS table combines
// therefore depends on the panel: with c1's four barcodes a workgroup's popular third falls on 256 keys and collapses
// fourfold; with c2 most keys of a workgroup are still distinct and the table mostly just batches them into the flush.
// 4096 slots hold every key a workgroup of that launch can produce at a load below three quarters.  A key that finds no
// slot within FLANK_LPROBE probes sits in a crowded stretch and goes to the global table at once: it costs the same
// single global atomic as a slot flushed with count 1, and the short probe run bounds the LDS traffic of the singleton
// tail.  32 KiB of keys + 16 KiB of 32-bit counts: three workgroups per CU.
#define FLANK_LCAP 4096
#define FLANK_LPROBE 4
#endif
#define FLANK_ACHUNK 256         // candidates the assign kernel stages in LDS at a time

struct FlankPanel {   // what the geometry needs of the panel
    int NP, S, Lb, k;
};

SMX_HD int flank_base_code(unsigned b) {   // A C G T -> 0 1 2 3, anything else (lower case, N, the zero padding) -> -1
    return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : -1;
}

SMX_HD uint64_t flank_key(uint64_t bits, unsigned flen, unsigned matched, unsigned p) {
    return bits | ((uint64_t)flen << SMX_FLANK_LEN_SHIFT) | ((uint64_t)matched << SMX_FLANK_MATCHED_SHIFT) |
           ((uint64_t)p << SMX_FLANK_PRIMER_SHIFT);
}
SMX_HD unsigned flank_key_len(uint64_t key) { return (unsigned)(key >> SMX_FLANK_LEN_SHIFT) & 31u; }
SMX_HD unsigned flank_key_primer(uint64_t key) { return (unsigned)(key >> SMX_FLANK_PRIMER_SHIFT) & 63u; }

// One hit: h = hits[read][2 * p + e], L = lens[read], win = the read's row of the ASCII window buffer (head window at
// [0, S), tail window at [S, 2 S)).  Returns 0 when the primer did not match (no hit), else the SMX_FLANK_* counter the
// hit goes to; *key is written for SMX_FLANK_COUNTED only.  Reads win only for L >= S and only inside [0, 2 S).
SMX_HD int flank_of_hit(const FlankPanel &P, const smx_hit &h, int p, int e, int L, const uint8_t *win, uint64_t *key) {
    if (h.pdist < 0) return 0;
    if (h.bbest == -2) return SMX_FLANK_PRUNED;
    if (L < P.S) return SMX_FLANK_SHORT_READ;
    const int S = P.S, W = P.Lb + P.k;
    const int j_end = h.first_end - (L - S);            // window position of the primer's first optimal end (end_geom)
    int flen = S - 1 - j_end;                           // the window ends where the end string ends
    if (j_end < 0 || flen < 0) flen = 0;                // (no hit the demux kernel writes: keeps every read in bounds)
    if (flen > W) flen = W;
    if (flen < P.Lb - P.k) return SMX_FLANK_SHORT_FLANK;
    uint64_t bits = 0;
    for (int t = 0; t < flen; t++) {
        const int j = j_end + 1 + t;
        // end B: the tail window as stored; end A: the reverse complement of the head window
        const int c = e ? flank_base_code(win[S + j]) : flank_base_code(win[S - 1 - j]);
        if (c < 0) return SMX_FLANK_AMBIGUOUS;
        bits |= (uint64_t)(e ? c : 3 - c) << (2 * t);
    }
    *key = flank_key(bits, (unsigned)flen, h.bbest >= 0, (unsigned)p);
    return SMX_FLANK_COUNTED;
}

// min over 0 <= j <= flen of NW(candidate, flank[:j]): edlib's SHW distance.  mw[c] = the candidate's match word for
// flank letter c (bit i: candidate letter i equals A C G T = 0 1 2 3), m = its length (1..26).  Myers' bit-vector
// column step with +1 entering row 0 (the flank's start is fixed); bits above m - 1 hold garbage that never flows down.
SMX_HD int flank_shw(const uint32_t mw[4], int m, uint64_t bits, int flen) {
    uint32_t Pv = ~0u, Mv = 0;
    const uint32_t top = 1u << (m - 1);
    int score = m, best = m;
    for (int t = 0; t < flen; t++, bits >>= 2) {
        const unsigned c = (unsigned)bits & 3u;
        const uint32_t Eq = c & 2u ? (c & 1u ? mw[3] : mw[2]) : (c & 1u ? mw[1] : mw[0]);
        const uint32_t Xv = Eq | Mv;
        const uint32_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        uint32_t Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
        score += (Ph & top) ? 1 : 0;
        score -= (Mh & top) ? 1 : 0;
        best = score < best ? score : best;
        Ph = (Ph << 1) | 1u;
        Mh <<= 1;
        Pv = Mh | ~(Xv | Ph);
        Mv = Ph & Xv;
    }
    return best;
}

struct FlankBest { int best, first, ntied; };   // least distance <= k (-1: none), first candidate that attains it, how many do

// One candidate more for a key's running result; `index` = the candidate's index in the caller's order (ascending calls).
SMX_HD void flank_take(FlankBest &r, int d, int k, int index) {
    if (d > k) return;
    if (r.best < 0 || d < r.best) { r.best = d; r.first = index; r.ntied = 1; }
    else if (d == r.best) r.ntied++;
}

}  // namespace smx
#endif
