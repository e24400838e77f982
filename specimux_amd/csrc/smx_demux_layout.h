// smx_demux_layout.h -- what the demux kernel and the host that launches it (smx_panel.cpp) must agree on: the LDS layout
// of a tile (make_layout) with its records, and the table of the kernel's instantiations.  Host/device code, no HIP
// intrinsics; the only header of the kernel that the host includes.
#ifndef SMX_DEMUX_LAYOUT_H
#define SMX_DEMUX_LAYOUT_H
#include "smx.h"

namespace smx {

// Tile geometry of the two-primer default-flags kernel (SP = 2): reads per tile, and the resident workgroups per CU it is
// built for.  Five: its tile is 31.5 KB of LDS (five of them fit a CU: tools/ubench/lds_residency.hip) and the register
// allocator is held to 96 VGPRs (8 values spilled).  Measured: 56-read tiles at four per CU 0.255 ms, at five 0.228 ms.
#ifndef SMX_SP2_R
#define SMX_SP2_R 64
#define SMX_SP2_WG 5
#endif

// LDS-resident per (read, primer, end) record.
struct HitL {
    int tail_end;       // reference coord: max optimal end over all within-k barcodes (slots mode), valid if bbest >= 0
    short nloc;
    short ntied;
    short first_tied;   // local index in the primer's barcode list
    signed char pdist;  // -1 no primer match (primers <= 64 nt)
    signed char bbest;  // -1 none, -2 not searched (barcodes <= 32 nt)
    unsigned char jstar;   // window position of the first optimal primer end
    unsigned char fs_j;    // window position of its start (need_starts only)
    unsigned char flags;   // bit0: orientation vote, bit1: barcode search needed
    unsigned char pad;
};
static_assert(sizeof(HitL) == 16, "HitL layout");

struct TileLayout {   // byte offsets into dynamic LDS
    int tacc, ppeq, prpeq, bpeq, bsre, lut, pmeta, codes, namask, lens, ocnt, rflag, hits, masks, tiem, bres, dmask, ents, offsA, offsB, queue, emit, opsL, aggr, etail,
        hmap, clist, pmask, hcand, total;
    int NI;      // per-alignment records a tile keeps: R * H (dense) or the compact capacity
    int CS;      // bytes per code row (odd number of dwords: conflict-free column reads across rows)
    int lNPs, lNBs;  // their log2
    int NPs, NBs;  // power-of-two strides of the transposed Peq tables: entry [code][pattern]
    int G, logG;   // barcode slots per (hit) group: power of two >= maxB
    int MBW;     // tie-mask words per hit
    int BSP;     // bit-sliced table: words per primer
    int CAPH, CAPE;  // hits / (hit, location) entries processed per barcode round
};

struct EntL {   // one optimal primer location of one searched hit = one barcode target
    unsigned short hit;     // r * H + h
    unsigned short slot;    // first bres slot of the hit in this round
    unsigned char tj0;      // window position of the first target base
    unsigned char loc_ord;  // ordinal of the location (ascending end)
    unsigned char ncol;     // target columns available (capped)
    unsigned char ok;       // 0: target empty or rejected by the prefilter rule
    short delta;            // reference coordinate of window position j at this location = j + base - delta (bc_geom)
    short pad;
};
static_assert(sizeof(EntL) == 12, "EntL layout");

// the scorer looks at the candidates of matched alignments only (panels with more than two primer pairs)
__host__ __device__ inline bool layout_cfilt(int H, int ncand) { return H <= 64 && ncand <= 64 && ncand > 4; }
__host__ __device__ inline bool layout_tie_in_rec(int MBW, int slots, int tails) { return MBW == 1 && !slots && !tails; }
#define OCNT_NA 0x8000

template <typename PW>
__host__ __device__ inline TileLayout make_layout(int NP, int NB, int S, int R, int maxB, int need_starts,
                                                    int npmeta, int kidx, int slots, int bs, int ncand, int cap_hits = 0,
                                                    int cap_ents = 0, int nitems = 0, int tails = 1, int nbstab = -1) {
    // nitems > 0: compact mode.  The tile keeps per-alignment state (hit record, end mask, scan slots) for at most nitems
    // of its R * H alignments -- the ones the prescan's match words flag -- plus one shared "no match" record; hmap maps
    // (read, alignment) to its record.  Panels with many primers spend most of their LDS on alignments that never match.
    TileLayout t;
    int H = 2 * NP, MW = (S + 31) / 32;
    t.CS = 4 * (((S + 3) / 4) | 1);
    t.NPs = 1; t.lNPs = 0; while (t.NPs < NP) { t.NPs <<= 1; t.lNPs++; }   // table index = (code << log2) | pattern:
    t.NBs = 1; t.lNBs = 0; while (t.NBs < NB) { t.NBs <<= 1; t.lNBs++; }   // no integer multiply in the inner loops
    t.G = 1; t.logG = 0;
    while (t.G < maxB) { t.G <<= 1; t.logG++; }
    t.MBW = (maxB + 31) / 32;
    // barcode rounds.  slots mode (--trim tails, parity dumps): one 4-byte atomicMin slot per (hit, barcode),
    // at most 16 KiB worth of hits per round.  lean mode: per hit only (k+1) x MBW words of "barcodes seen at
    // distance d" bitmasks, at most 4 KiB per round.
    const int sentinel = nitems > 0 ? 1 : 0;
    t.NI = nitems > 0 ? nitems : R * H;
    int dense = t.NI;
    // (compact mode: up to 8 KiB, so that the searched hits of a 64-read tile usually go in ONE round -- the several-round
    // path has serial bookkeeping)
    int fit = slots ? (16 * 1024) / (t.G * 4) : ((nitems > 0 ? 8 : 3) * 1024) / ((kidx + 1) * t.MBW * 4);
    t.CAPH = dense < fit ? dense : (fit < 1 ? 1 : fit);
    t.CAPE = t.CAPH + t.CAPH / 4 < 256 ? 256 : t.CAPH + t.CAPH / 4;   // >= 256 = max locations of one hit (progress)
    if (nitems > 0) t.CAPE = t.CAPH + t.CAPH / 2 < 256 ? 256 : t.CAPH + t.CAPH / 2;   // (noisy reads of a wide window: several optimal ends per hit)
    if (cap_hits > 0 && cap_hits < t.CAPH) t.CAPH = cap_hits;          // test hook: many small rounds
    if (cap_ents >= S && cap_ents < t.CAPE) t.CAPE = cap_ents;         // (a hit has at most S locations)
    // Order: regions whose offsets depend on the tile geometry only (R, S) come first -- compile-time constants in the
    // default-flags kernel --, then the per-alignment regions (R * 2 NP or the compact capacity), the panel tables last.
    int o = 0;
    t.tacc = o;  o += 11 * 8 + 8;
    t.lut = o;   o += 512;
    t.aggr = o;  o += 12 * 4;
    o = (o + 15) & ~15;
    t.codes = o; o += R * 2 * t.CS;
    t.namask = o; o += R * 2 * MW * 4;         // per code row: bit j set = code[j] is not A/C/G/T
    t.lens = o;  o += 2 * R * 4;               // double-buffered: the next tile is encoded while this one is scored
    t.ocnt = o;  o += 2 * R * 4;               // per read: forward votes | OCNT_NA (a window holds something other than upper-case
                                               // ACGT: scalar primer scan) | reverse votes << 16; double-buffered
    t.rflag = o;                               // (round 3: the flag is bit 15 of ocnt, no region of its own)
    o = (o + 7) & ~7;
    const bool cf = layout_cfilt(H, ncand);
    t.pmask = o; o += cf ? R * 8 : 0;          // per read: bit h = alignment h found its primer (scorer: which candidates to look at)
    o = (o + 15) & ~15;
    t.hits = o;  o += (t.NI + sentinel) * (int)sizeof(HitL);
    // one tie-mask word per record and nothing else wanting HitL::tail_end (it belongs to slots mode and --trim tails): the word
    // lives there, no array of its own
    t.tiem = o;  o += layout_tie_in_rec(t.MBW, slots, tails) ? 0 : (t.NI + sentinel) * t.MBW * 4;
    t.clist = o; o += nitems > 0 ? ((t.NI + 1) & ~1) * 2 : 0;       // record -> read * H + alignment
    // time-shared regions: {location entries} are dead after the barcode scan -> staged result records;
    // {primer end masks, scans, queue} are dead once the scorer starts -> its per-(read, candidate) trim shifts (Q8)
    t.bres = t.dmask = o; o += slots ? t.CAPH * t.G * 4 : t.CAPH * (kidx + 1) * t.MBW * 4;
    {
        int c = t.CAPE * (int)sizeof(EntL), d = R * 32;
        o = (o + 15) & ~15;
        t.ents = t.opsL = o; o += c > d ? c : d;
    }
    t.etail = o; o += (bs && !slots && tails) ? t.CAPE * 4 : 0;   // --trim tails on the lean path (BSV == 3): end of the kept alignment per entry
    t.masks = t.emit = o; o += t.NI * MW * 4;
    o = (o + 3) & ~3;
    t.offsA = o; o += ((t.NI + 2) & ~1) * 2;   // 16-bit scans: a tile has at most NI * S < 65536 locations
    t.offsB = o; o += ((t.NI + 2) & ~1) * 2 < 16 ? 16 : ((t.NI + 2) & ~1) * 2;   // (>= 16 bytes: the one-round path parks four wave sums here)
    t.queue = o; o += ((t.NI + 1) & ~1) * 2;
    if (o < t.emit + R * ncand * 4) o = t.emit + R * ncand * 4;
    o = (o + 7) & ~7;
    t.hmap = o;  o += nitems > 0 ? ((R * H + 1) & ~1) * 2 : 0;     // (read, alignment) -> record; t.NI = the shared "no match" record
    o = (o + 7) & ~7;
    t.hcand = o; o += cf ? H * 8 : 0;          // per alignment: the candidates (pair * 2 + orientation) it belongs to
    o = (o + 15) & ~15;
    t.ppeq = o;  o += t.NPs * 16 * (int)sizeof(PW);
    t.prpeq = o; o += (need_starts ? t.NPs * 16 * (int)sizeof(PW) : 0);
    t.bpeq = o;  o += (bs && !slots) ? 0 : t.NBs * 16 * 4;
    t.BSP = 16 * 16 + 4;                        // words per (primer, 32-barcode word) block of the bit-sliced table (+4: bank skew)
    t.bsre = o;  o += (bs && !slots) ? (nbstab > 0 ? nbstab : NP) * t.MBW * t.BSP * 4 : 0;   // one table per distinct barcode list
    t.pmeta = o; o += npmeta * 4;
    t.total = (o + 15) & ~15;
    return t;
}

// The make_layout arguments that follow from a panel's sizes.  The host (smx_demux_lds_bytes: the LDS a launch reserves) and
// DemuxTile::setup (the LDS the kernel addresses) both take them from here; a specialised kernel passes its constants.
struct LayoutArgs { int npmeta, ncand, tails; };
__host__ __device__ __forceinline__ LayoutArgs layout_args(int NP, int NB, int n_pbc, int NPAIR, int trim) {
    return {6 * NP + 1 + n_pbc + NB + 3 * NPAIR, 2 * NPAIR, trim == SMX_TRIM_TAILS ? 1 : 0};
}

}  // namespace smx

// The kernel's instantiations, 20 of them at half a minute of compile time each, one row per (part, primer word bits,
// barcode scan variant BSV, dense / compact / redo mode CM, default-flags specialisation SP).  smx_demux.hip is compiled three
// times (-DSMX_PART=1 / 2 / 3, in parallel); each part instantiates the rows that name it.  A new instantiation is one row
// here plus the condition in demux_variant (smx_panel.cpp) that selects it.
#define SMX_DEMUX_VARIANTS(P1, P2, P3)                                                                           \
    P1(64, 0, 0, 0) P1(64, 1, 0, 0) P1(64, 2, 0, 0) P1(64, 3, 0, 0)   /* 64-bit primer words */                  \
    P1(32, 0, 0, 0) P1(32, 0, 1, 0) P1(32, 0, 2, 0)                   /* per-barcode scan */                     \
    P2(32, 1, 0, 0) P2(32, 1, 1, 0) P2(32, 1, 2, 0)                   /* bit-sliced scan, k <= 3 */              \
    P2(32, 2, 0, 0) P2(32, 2, 1, 0) P2(32, 2, 2, 0)                   /* bit-sliced scan, k 4..7 */              \
    P3(32, 3, 0, 0) P3(32, 3, 1, 0) P3(32, 3, 2, 0)                   /* the tails variant */                    \
    P3(32, 1, 0, 2) P3(32, 1, 1, 3) P3(32, 1, 1, 1) P3(32, 1, 0, 1)   /* the default-flags kernels */
struct DemuxVariant { int wbits, bsv, cm, sp; };
typedef unsigned smx_w32;
typedef unsigned long long smx_w64;
// the kernel of a row, from the part of smx_demux.hip that instantiates it (nullptr from the other two parts)
extern "C" const void *smx_demux_fn_p1(DemuxVariant v);
extern "C" const void *smx_demux_fn_p2(DemuxVariant v);
extern "C" const void *smx_demux_fn_p3(DemuxVariant v);
#endif
