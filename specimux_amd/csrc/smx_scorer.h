// smx_scorer.h -- phase 4 of the demux kernel: from a read's hit records (ReadCtx) to its smx_op records (Emitter).
// Device code; it knows nothing of the tile (smx_demux_tile.h) beyond those two structures.
#ifndef SMX_SCORER_H
#define SMX_SCORER_H
#include "smx_internal.h"
#include "smx_align_core.h"
#include "smx_demux_layout.h"

namespace smx {

// Scorer helpers (phase 4).  Everything is indexed, nothing is string keyed.
// Small per-panel tables staged in LDS (the scorer and the barcode scan read them constantly).
struct LPanel {
    const int *pm, *pk, *pdir, *pfidx, *pbc_off, *pbc, *bm, *pair_f, *pair_r, *pair_pool, *bstab;
};

struct ReadCtx {
    const DevPanel *P;
    LPanel LP;
    const HitL *hits;          // this read's H records (compact mode: the tile's records, indexed through hmap)
    const unsigned *tiem;      // the records' tie bitmasks (barcodes at the best distance): word w of record i = tiem[i * tstr + w]
    int tstr;
    const unsigned short *hmap;   // compact mode: this read's alignment -> record; nullptr: record = alignment
    const unsigned long long *hcand;   // per alignment: bitmask of the candidates it belongs to; nullptr: look at every candidate
    int trim, derep;              // the panel's --trim / --dereplicate (compile-time constants in the default-flags kernel)
    int npair;                    // primer pairs (a constant 1 in the two-primer kernel)
    unsigned long long pm;        // this read's alignments with a primer match (bit h)
    unsigned long long live;      // candidates (pair * 2 + orientation) worth looking at: one of their alignments matched, and
                                  // the orientation is allowed; all ones when there is no candidate table (hcand == nullptr)
    // Panels with many primer pairs: a candidate scores > 0 only if one of its two alignments found its primer, so only the
    // candidates of this read's matched alignments are looked at (a handful of the 2 * NPAIR).  Nothing else changes: every
    // quantity the scorers compute is a function of the candidates with a positive score.
    __device__ __forceinline__ void set_live(int ori) {
        live = ~0ull;
        if (hcand) {
            live = 0ull;
            for (unsigned long long m = pm; m; m &= m - 1ull) live |= hcand[__ffsll((long long)m) - 1];
            if (ori == 2) live &= 0xAAAAAAAAAAAAAAAAull;        // reverse-complement candidates only (odd ids)
            else if (ori == 1) live &= 0x5555555555555555ull;
        }
    }
    __device__ __forceinline__ bool cand_live(int ci) const { return !hcand || ((live >> ci) & 1ull); }
    int MBW;
    __device__ __forceinline__ int rec(int h) const { return hmap ? (int)hmap[h] : h; }
    __device__ __forceinline__ const HitL &hit(int h) const { return hits[rec(h)]; }
    int L, S;
    EndGeom g;
};

struct CandView {
    int f, r, o;               // forward primer, reverse primer, orientation 0 = as read, 1 = reverse complement
    int h1, h2;                // hit indices (primer*2 + end)
    bool p1, p2, b1, b2;
    int p1d, p2d, b1d, b2d;
};

__device__ __forceinline__ CandView cand_view(const ReadCtx &c, int pair, int o) {
    CandView v;
    v.f = c.LP.pair_f[pair];
    v.r = c.LP.pair_r[pair];
    v.o = o;
    v.h1 = v.f * 2 + (o == 0 ? 0 : 1);   // forward primer: end A (of rs) when the read is kept as is
    v.h2 = v.r * 2 + (o == 0 ? 1 : 0);
    const HitL &a = c.hit(v.h1);
    const HitL &b = c.hit(v.h2);
    v.p1 = a.pdist >= 0;
    v.p2 = b.pdist >= 0;
    v.b1 = v.p1 && a.bbest >= 0;
    v.b2 = v.p2 && b.bbest >= 0;
    v.p1d = v.p1 ? a.pdist : -1;
    v.p2d = v.p2 ? b.pdist : -1;
    v.b1d = v.b1 ? a.bbest : -1;
    v.b2d = v.b2 ? b.bbest : -1;
    return v;
}

__device__ __forceinline__ int cand_score(const CandView &v) {   // demultiplex.py:226-236
    if (v.p1 && v.p2 && v.b1 && v.b2) return 5;
    if (v.p1 && v.p2 && (v.b1 || v.b2)) return 4;
    if ((v.p1 || v.p2) && (v.b1 || v.b2)) return 3;
    if (v.p1 && v.p2) return 2;
    if (v.p1 || v.p2) return 1;
    return 0;
}

// next tied barcode (local index >= from) of hit h in canonical order; -1 when exhausted.  (Find-first-set on the tie
// mask words: the scorers enumerate tie sets in nested loops, and a bit-by-bit scan of up to maxB positions per call was
// most of the general scorer's instruction stream.)
__device__ inline int next_tied(const ReadCtx &c, int h, int from) {
    int p = h >> 1;
    int nb = c.LP.pbc_off[p + 1] - c.LP.pbc_off[p];
    if (from >= nb) return -1;
    const unsigned *tm = c.tiem + c.rec(h) * c.tstr;
    int w = from >> 5;
    unsigned word = tm[w] & (~0u << (from & 31));
    for (;;) {
        if (word) {
            const int i = w * 32 + __ffs((int)word) - 1;
            return i < nb ? i : -1;
        }
        if (++w >= c.MBW) return -1;
        word = tm[w];
    }
}
__device__ __forceinline__ int global_bc(const ReadCtx &c, int h, int local) {
    return c.LP.pbc[c.LP.pbc_off[h >> 1] + local];
}
__device__ inline bool tied_has_global(const ReadCtx &c, int h, int gb) {
    for (int i = next_tied(c, h, 0); i >= 0; i = next_tied(c, h, i + 1))
        if (global_bc(c, h, i) == gb) return true;
    return false;
}

// Specimens.specimen_for_exact_match (databases.py:232-245): first specimen in file order.
// One 32-byte load in the usual case -- the (b1, b2) cell holds the first specimen's whole record (masks, pool, next) --
// instead of three dependent ones (head of the chain, its primer masks, its pool): the scorer wave sits on a tile's
// critical path and every dependent global load is most of a microsecond.  The flat tables are gone from the device:
// five fewer pointers held in (spilled) SGPRs.
// (load_specrec: the record's two 16-byte halves are requested together and pass through one point.  A plain struct copy
// is taken apart by the compiler: `spec` first, the masks once it is known to be >= 0, `next` and `pool` where they are
// used -- up to four dependent round trips for one 32-byte record.)
__device__ __forceinline__ SpecRec load_specrec(const SpecRec *p) {
    static_assert(sizeof(SpecRec) == 32 && offsetof(SpecRec, spec) == 16, "SpecRec layout");   // (tables are 16-byte aligned: blob_add)
    uint4 a = ((const uint4 *)p)[0], b = ((const uint4 *)p)[1];
    asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w), "+v"(b.x), "+v"(b.y), "+v"(b.z), "+v"(b.w));
    SpecRec rec;
    rec.p1m = ((unsigned long long)a.y << 32) | a.x; rec.p2m = ((unsigned long long)a.w << 32) | a.z;
    rec.spec = (int)b.x; rec.next = (int)b.y; rec.pool = (int)b.z; rec.pad = (int)b.w;
    return rec;
}
__device__ inline int specimen_exact(const DevPanel *P, int gb1, int gb2, int f, int r, int *pool_out = nullptr) {
    SpecRec rec = load_specrec(&P->pairrec[(size_t)gb1 * P->NB + gb2]);
    while (rec.spec >= 0) {
        if (((rec.p1m >> f) & 1) && ((rec.p2m >> r) & 1)) {
            if (pool_out) *pool_out = rec.pool;
            return rec.spec;
        }
        if (rec.next < 0) break;
        rec = load_specrec(&P->specrec[rec.next]);
    }
    return -1;
}
// Specimens.specimens_for_barcodes_and_primers (databases.py): how many specimens carry (b1, b2) with these primers, and
// the first of them in file order
__device__ inline void specimens_for(const DevPanel *P, int gb1, int gb2, int f, int r, int &first, int &cnt) {
    SpecRec rec = load_specrec(&P->pairrec[(size_t)gb1 * P->NB + gb2]);
    while (rec.spec >= 0) {
        if (((rec.p1m >> f) & 1) && ((rec.p2m >> r) & 1)) {
            cnt++;
            if (first < 0 || rec.spec < first) first = rec.spec;
        }
        if (rec.next < 0) break;
        rec = load_specrec(&P->specrec[rec.next]);
    }
}

// Trim extents of a candidate whose stored locations were already shifted by `cum` (Q8).
// models.py:278-319 with p1 locations mirrored by AlignmentResult.reversed (models.py:58-63).
__device__ inline void cand_extent(const ReadCtx &c, const CandView &v, int cum, int &s, int &e) {
    const DevPanel *P = c.P;
    int L = c.L;
    const HitL &a = c.hit(v.h1);
    const HitL &b = c.hit(v.h2);
    // first primer location in reference coordinates of the searched string
    int a_end = 0, a_start = 0, b_end = 0, b_start = 0;
    if (v.p1) { a_end = (int)a.jstar - c.g.j_lo + c.g.shift; a_start = (int)a.fs_j - c.g.j_lo + c.g.shift; }
    if (v.p2) { b_end = (int)b.jstar - c.g.j_lo + c.g.shift; b_start = (int)b.fs_j - c.g.j_lo + c.g.shift; }
    s = 0; e = L;
    if (c.trim == SMX_TRIM_BARCODES) {
        if (v.p1) s = (L - a_end - 1) - cum;
        if (v.p2) e = (b_end + 1) - cum;
    } else if (c.trim == SMX_TRIM_PRIMERS || c.trim == SMX_TRIM_TAILS) {
        int ps = 0, pe = L;
        if (v.p1) ps = (L - a_start - 1) + 1 - cum;
        if (v.p2) pe = b_start - cum;
        if (c.trim == SMX_TRIM_PRIMERS) { s = ps; e = pe; }
        else {
            if (v.b1) s = (L - a.tail_end - 1) - cum;
            else { s = ps - P->bmax; if (s < 0) s = 0; }
            if (v.b2) e = (b.tail_end + 1) - cum;
            else { e = pe + P->bmax; if (e > L) e = L; }
        }
    }
}

struct Emitter {
    const ReadCtx *c;
    smx_op *primary;           // LDS staging slot of this read's first record
    smx_op *extra;
    unsigned extra_cap;
    unsigned *n_extra;
    unsigned long long *counts;
    int *cum;                  // LDS, one int per candidate of this read: the trim shift its earlier emissions have added up (Q8)
    int *aggr;                 // LDS block aggregates
    unsigned read;
    int n;                     // ops emitted so far
    bool matched;
    bool overflow;
};

// create_write_operation (demultiplex.py:30-103) in index form.  has_v = false: the record of a read without any
// candidate; `v` is then a view the caller happens to have (or a dummy) and is not looked at.  (A `const CandView *` that
// may be null kept the caller's view in scratch memory: every field the record takes was a dependent scratch load on the
// scorer wave's critical path.)
__device__ inline void emit_op(Emitter &E, const CandView &v, bool has_v, int cand_id, int sample, int rtype, int pool,
                               int barcode, unsigned xflags) {
    const ReadCtx &c = *E.c;
    smx_op op;
    op.read = E.read;
    op.n_ops = 0;
    op.flags = (unsigned char)xflags;
    op.barcode = (short)barcode;
    int s = 0, e = c.L;
    if (has_v) {
        op.dist[0] = (int8_t)v.p1d; op.dist[1] = (int8_t)v.b1d; op.dist[2] = (int8_t)v.b2d; op.dist[3] = (int8_t)v.p2d;
        op.p1 = (short)(v.p1 ? v.f : -1);
        op.p2 = (short)(v.p2 ? v.r : -1);
        if (v.o) op.flags |= SMX_OPF_REVERSE;
    } else {
        op.dist[0] = op.dist[1] = op.dist[2] = op.dist[3] = -1;
        op.p1 = op.p2 = -1;
    }
    bool fallback = false;
    if (c.trim != SMX_TRIM_NONE) {
        if (has_v) {
            // Q8: the same CandidateMatch emitted earlier already had its locations shifted by the trim start of each of
            // those emissions.  One running sum per candidate: any number of emissions per read (a tie storm at a large
            // index distance emits one record per tied specimen, hundreds for one read).
            const int cum = E.cum[cand_id];
            cand_extent(c, v, cum, s, e);
            if (s < e) E.cum[cand_id] = cum + s;
        }
        if (s >= e) { fallback = true; s = 0; e = c.L; }   // Q12
    }
    op.trim_start = s;
    op.trim_end = e;
    if (fallback) {
        op.flags |= SMX_OPF_TRIM_EMPTY;
        op.sample = -1; op.pool = -1; op.p1 = -1; op.p2 = -1; op.barcode = -1;
        op.rtype = SMX_R_UNKNOWN;
    } else {
        op.sample = sample;
        op.pool = (short)pool;
        op.rtype = (unsigned char)rtype;
    }
    if (rtype == SMX_R_FULL || rtype == SMX_R_DEREP_FULL) E.matched = true;
    // counters
    int cls = (op.rtype == SMX_R_UNKNOWN) ? 2 : ((op.rtype == SMX_R_PARTIAL_FWD || op.rtype == SMX_R_PARTIAL_REV) ? 1 : 0);
    atomicAdd(&E.aggr[3 + cls], 1);
    if (cls == 0 && op.sample >= 0) atomicAdd(&E.counts[SMX_CNT_SPECIMEN0 + op.sample], 1ull);
    if (E.n == 0) {
        *E.primary = op;
    } else {
        unsigned slot = atomicAdd(E.n_extra, 1u);
        if (slot < E.extra_cap) E.extra[slot] = op;
    }
    E.n++;
    if (E.n > 0xFFFF) E.overflow = true;   // n_ops is 16 bits wide
}

// resolve_specimen for a non-full candidate (demultiplex.py:576-589) -> emits.
__device__ inline void emit_partial_or_unknown(Emitter &E, const CandView &v, int cand_id, int pool) {
    const ReadCtx &c = *E.c;
    if (v.b1 && !v.b2 && c.hit(v.h1).ntied == 1)
        emit_op(E, v, true, cand_id, -1, SMX_R_PARTIAL_FWD, pool, global_bc(c, v.h1, c.hit(v.h1).first_tied), 0);
    else if (v.b2 && !v.b1 && c.hit(v.h2).ntied == 1)
        emit_op(E, v, true, cand_id, -1, SMX_R_PARTIAL_REV, pool, global_bc(c, v.h2, c.hit(v.h2).first_tied), 0);
    else
        emit_op(E, v, true, cand_id, -1, SMX_R_UNKNOWN, pool, -1, 0);
}

// Iterate the best-scoring candidates in find_candidate_matches order.
#define FOR_BEST_CANDS(c, ori, best, ...)                                               \
    for (int _pair = 0; _pair < (c).npair; _pair++)                                      \
        for (int _o = 0; _o < 2; _o++) {                                                 \
            if ((_o == 0 && (ori) == 2) || (_o == 1 && (ori) == 1)) continue;            \
            if (!(c).cand_live(_pair * 2 + _o)) continue;                                \
            CandView v = cand_view((c), _pair, _o);                                      \
            if (!(v.p1 || v.p2)) continue;                                               \
            if (cand_score(v) != (best)) continue;                                       \
            int cand_id = _pair * 2 + _o;                                                \
            int cand_pool = (c).LP.pair_pool[_pair];                                     \
            (void)cand_id; (void)cand_pool;                                              \
            __VA_ARGS__                                                                  \
        }

// key for dereplicate_matches' specimen groups (demultiplex.py:371-378); all lexicographic, small ints
__device__ __forceinline__ int key_full(const LPanel &P, const CandView &v) {
    return ((v.b1d + v.b2d) << 20) | ((v.p1d + v.p2d) << 12) | (P.pfidx[v.f] + P.pfidx[v.r]);
}
__device__ __forceinline__ int key_partial(const LPanel &P, const CandView &v, bool fwd) {   // :442-463
    int cnt = (v.p1 ? 1 : 0) + (v.p2 ? 1 : 0);
    int pd = (v.p1 ? v.p1d : 0) + (v.p2 ? v.p2d : 0);
    int fi = (v.p1 ? P.pfidx[v.f] : 0) + (v.p2 ? P.pfidx[v.r] : 0);
    return ((fwd ? v.b1d : v.b2d) << 24) | ((2 - cnt) << 22) | (pd << 12) | fi;
}
__device__ __forceinline__ int key_unknown(const LPanel &P, const CandView &v) {             // :502-528
    int cnt = (v.p1 ? 1 : 0) + (v.p2 ? 1 : 0);
    int pd = (v.p1 ? v.p1d : 0) + (v.p2 ? v.p2d : 0);
    int fi = (v.p1 ? P.pfidx[v.f] : 999) + (v.p2 ? P.pfidx[v.r] : 999);
    return ((2 - cnt) << 22) | (pd << 12) | fi;
}

// does candidate v map some tied (b1,b2) combination to specimen `spec`?  (spec = -1: to ANY specimen)
__device__ inline bool cand_has_specimen(const ReadCtx &c, const CandView &v, int spec) {
    for (int i = next_tied(c, v.h1, 0); i >= 0; i = next_tied(c, v.h1, i + 1))
        for (int j = next_tied(c, v.h2, 0); j >= 0; j = next_tied(c, v.h2, j + 1)) {
            int s = specimen_exact(c.P, global_bc(c, v.h1, i), global_bc(c, v.h2, j), v.f, v.r);
            if (s >= 0 && (spec < 0 || s == spec)) return true;
        }
    return false;
}

// Fast scorer of the hot kernel: handles "no candidate" and "exactly one candidate at the best score, no
// barcode tie".  Every dereplication group then has one member and the reference's machinery reduces to a
// single emission.  Returns false for everything else (several best candidates, ties): the caller then runs
// score_general, the reference's selection / dereplication in full, for that read.
// `G` lanes (a power of two, consecutive, `sub` = this lane's index among them) share one read: the candidate loops are
// split over them and reduced by xor-shuffles (tiles of panels with many primers hold fewer than 64 reads, so the scorer
// wave has lanes to spare, and with 10 candidates the loops are most of its instruction stream); everything after the
// reductions -- one record in the usual case -- is done by sub-lane 0, the others return true at once.
__device__ inline bool score_fast(Emitter &E, int ori, int sub, int G) {
    const ReadCtx &c = *E.c;
    const DevPanel *P = c.P;
    // ---- select_best_matches (demultiplex.py:216-259): best score, how many carry it, the first of them
    int best = 0, nbest = 0, first = 0x7FFF;
    const int ncand = c.npair * 2;
    const unsigned long long live = c.live;   // (ReadCtx::set_live)
    if (c.hcand) {
        for (unsigned long long m = live; m; m &= m - 1ull) {
            const int ci = __ffsll((long long)m) - 1;
            if ((ci & (G - 1)) != sub) continue;
            CandView v = cand_view(c, ci >> 1, ci & 1);
            int sc = cand_score(v);
            if (sc > best) { best = sc; nbest = 1; first = ci; }
            else if (sc == best) { nbest++; first = ci < first ? ci : first; }
        }
    } else
    for (int ci = sub; ci < ncand; ci += G) {
        const int pair = ci >> 1, o = ci & 1;
        if ((o == 0 && ori == 2) || (o == 1 && ori == 1)) continue;
        CandView v = cand_view(c, pair, o);
        int sc = cand_score(v);
        if (sc > best) { best = sc; nbest = 1; first = ci; }
        else if (sc == best) { nbest++; first = ci < first ? ci : first; }
    }
    for (int d = 1; d < G; d <<= 1) {
        const int ob = __shfl_xor(best, d, 64), on = __shfl_xor(nbest, d, 64), of = __shfl_xor(first, d, 64);
        if (ob > best) { best = ob; nbest = on; first = of; }
        else if (ob == best) { nbest += on; first = of < first ? of : first; }
    }
    const int only_pair = first >> 1, only_o = first & 1;
    // The divergent case analysis below only picks the parameters of the ONE record this read emits; the record
    // itself is built once, after the lanes have converged again (emit_op is by far the longest piece of code here).
    bool has_v = true;
    int pair = only_pair, o = only_o, sample = -1, rtype = SMX_R_UNKNOWN, barcode = -1;
    const bool lead = sub == 0;   // the lane that analyses the winner and emits; its partners only take part in the shuffles
    unsigned xflags = 0;
    int more1 = -1, more2 = -1, more3 = -1;   // further specimens of a tied full match
    int repeat = 1;                           // identical UNKNOWN records (one per tied barcode of a partial match)
    int spool = -2;                           // the specimen's pool when the lookup already brought it along
    if (best == 0) {   // no candidate at all (demultiplex.py:202-210)
        has_v = false; pair = 0; o = 0;
    } else if (best <= 2 && nbest > 1) {
        // several primer-only candidates (typically both orientations of one pair): no barcode logic involved.
        // dereplicate=best -> dereplicate_unknown_matches: stable minimum of (-primer_count, primer_dist, file index);
        // dereplicate=none -> every best candidate is written as UNKNOWN (demultiplex.py:181-197, :480-538): general path
        if (c.derep == SMX_DEREP_NONE) return sub != 0;
        int wkey = 0x7FFFFFFF, wci = 0x7FFF;
        for (int ci = sub; ci < ncand; ci += G) {
            const int pr = ci >> 1, oo = ci & 1;
            if ((oo == 0 && ori == 2) || (oo == 1 && ori == 1)) continue;
            if (!((live >> ci) & 1ull)) continue;
            CandView v = cand_view(c, pr, oo);
            if (cand_score(v) != best) continue;
            int k = key_unknown(c.LP, v);
            if (k < wkey) { wkey = k; wci = ci; }   // first minimum in candidate order within this lane's stride
        }
        for (int d = 1; d < G; d <<= 1) {
            const int ok = __shfl_xor(wkey, d, 64), oc = __shfl_xor(wci, d, 64);
            if (ok < wkey || (ok == wkey && oc < wci)) { wkey = ok; wci = oc; }
        }
        pair = wci >> 1; o = wci & 1;
    } else if (best <= 4 && nbest > 1) {
        // several partial candidates (typically the pairs that share one primer, when only that primer's end of the read is
        // good).  dereplicate_partial_matches (demultiplex.py:396-477) groups them by (direction, barcode); when every one
        // of them has a single untied barcode and it is the same (direction, barcode) for all, there is one group and its
        // winner -- stable minimum of key_partial -- is the one record.  Anything else: the general scorer.
        if (!lead) return true;
        if (c.derep != SMX_DEREP_BEST) return false;
        int gdir = -1, ggb = -1, wkey = 0x7FFFFFFF, wci = -1;
        for (int ci = 0; ci < ncand; ci++) {
            if (!((live >> ci) & 1ull)) continue;
            if (((ci & 1) == 0 && ori == 2) || ((ci & 1) == 1 && ori == 1)) continue;
            const CandView v = cand_view(c, ci >> 1, ci & 1);
            if (cand_score(v) != best) continue;
            const bool fwd = v.b1;
            const int h = fwd ? v.h1 : v.h2;
            const HitL &x = c.hit(h);
            if (x.ntied != 1) return false;
            const int gb = global_bc(c, h, x.first_tied);
            if (gdir < 0) { gdir = fwd ? 1 : 0; ggb = gb; }
            else if (gdir != (fwd ? 1 : 0) || ggb != gb) return false;
            const int k = key_partial(c.LP, v, fwd);
            if (k < wkey) { wkey = k; wci = ci; }
        }
        pair = wci >> 1; o = wci & 1;
        const CandView w = cand_view(c, pair, o);   // resolve_specimen of the winner (demultiplex.py:576-589)
        if (w.b1 && !w.b2) { rtype = SMX_R_PARTIAL_FWD; barcode = ggb; }
        else if (w.b2 && !w.b1) { rtype = SMX_R_PARTIAL_REV; barcode = ggb; }
    } else {
        if (!lead) return true;
        if (nbest != 1) return false;
        const CandView v = cand_view(c, pair, o);
        const HitL &a = c.hit(v.h1), &b = c.hit(v.h2);
        const bool t1 = !v.b1 || a.ntied == 1, t2 = !v.b2 || b.ntied == 1;
        if (best <= 2) {
            // dereplicate_unknown_matches / resolve_specimen: UNKNOWN either way
        } else if (best <= 4) {   // one (direction, barcode) group: resolve_specimen (demultiplex.py:576-589)
            if (!(t1 && t2)) {
                // tied barcodes on the one end that has any: dereplicate_partial_matches makes one group per tied barcode,
                // each with this candidate as its only member, and resolve_specimen turns each into UNKNOWN (the barcode is
                // ambiguous): ntied identical records
                if (c.derep != SMX_DEREP_BEST) return false;
                repeat = v.b1 ? a.ntied : b.ntied;
            }
            else if (v.b1 && !v.b2) { rtype = SMX_R_PARTIAL_FWD; barcode = global_bc(c, v.h1, a.first_tied); }
            else if (v.b2 && !v.b1) { rtype = SMX_R_PARTIAL_REV; barcode = global_bc(c, v.h2, b.first_tied); }
        } else if (c.derep != SMX_DEREP_BEST) {
            // --dereplicate none: resolve_specimen's full branch (demultiplex.py:555-575) for untied barcodes --
            // specimens_for_barcodes_and_primers in file order: one -> FULL_MATCH, several -> the first + MULTIPLE
            if (!(t1 && t2)) return false;
            const int g1 = global_bc(c, v.h1, a.first_tied), g2 = global_bc(c, v.h2, b.first_tied);
            int first = -1, cnt = 0;
            specimens_for(P, g1, g2, v.f, v.r, first, cnt);
            if (cnt > 0) { sample = first; rtype = cnt > 1 ? SMX_R_MULTIPLE : SMX_R_FULL; }
            else xflags = SMX_OPF_NO_SPECIMEN;
        } else {
            if (t1 && t2) {
                int spec = specimen_exact(P, global_bc(c, v.h1, a.first_tied), global_bc(c, v.h2, b.first_tied), v.f, v.r, &spool);
                if (spec >= 0) { sample = spec; rtype = SMX_R_DEREP_FULL; }
                else xflags = SMX_OPF_NO_SPECIMEN;
            } else {
                // one candidate, tied barcodes (by far the most frequent reason to leave the single-record path):
                // dereplicate_matches (demultiplex.py:262-393) with one member per group = one DEREP_FULL record per
                // distinct specimen among the tied (b1, b2) combinations, in first-appearance order
                int s0 = -1, s1 = -1, s2 = -1, s3 = -1, ns = 0;
                for (int i = next_tied(c, v.h1, 0); i >= 0; i = next_tied(c, v.h1, i + 1))
                    for (int j = next_tied(c, v.h2, 0); j >= 0; j = next_tied(c, v.h2, j + 1)) {
                        int sp = specimen_exact(P, global_bc(c, v.h1, i), global_bc(c, v.h2, j), v.f, v.r);
                        if (sp < 0 || sp == s0 || sp == s1 || sp == s2 || sp == s3) continue;
                        if (ns == 4) return false;   // more groups than this path keeps: the general scorer takes over
                        if (ns == 0) s0 = sp; else if (ns == 1) s1 = sp; else if (ns == 2) s2 = sp; else s3 = sp;
                        ns++;
                    }
                if (ns == 0) xflags = SMX_OPF_NO_SPECIMEN;
                else {
                    sample = s0; rtype = SMX_R_DEREP_FULL;
                    more1 = s1; more2 = s2; more3 = s3;
                }
            }
        }
    }
    if (!lead) return true;
    const CandView v = cand_view(c, pair, o);
    const int pool = !has_v ? -1 : (sample >= 0 ? (spool != -2 ? spool : P->specrec[sample].pool) : c.LP.pair_pool[pair]);
    emit_op(E, v, has_v, pair * 2 + o, sample, rtype, pool, barcode, xflags);   // (best == 0: the view of candidate 0, not looked at)
    for (int e = 1; e < repeat; e++) emit_op(E, v, true, pair * 2 + o, -1, SMX_R_UNKNOWN, pool, -1, 0);   // rare
    if (more1 >= 0) {   // rare
        for (int e = 0; e < 3; e++) {
            int sp = e == 0 ? more1 : (e == 1 ? more2 : more3);
            if (sp >= 0) emit_op(E, v, true, pair * 2 + o, sp, SMX_R_DEREP_FULL, P->specrec[sp].pool, -1, 0);
        }
    }
    return true;
}

// General scorer: the reference's selection / dereplication in full (reads score_fast declines, ~0.1 %).
__device__ inline void score_general(Emitter &E, int ori) {
    const ReadCtx &c = *E.c;
    const DevPanel *P = c.P;
    int best = 0;
    for (int pair = 0; pair < c.npair; pair++)
        for (int o = 0; o < 2; o++) {
            if ((o == 0 && ori == 2) || (o == 1 && ori == 1)) continue;
            if (!c.cand_live(pair * 2 + o)) continue;
            CandView v = cand_view(c, pair, o);
            int sc = cand_score(v);
            best = sc > best ? sc : best;
        }
    if (best == 0) {   // (not reached from the kernel: score_fast emits this record itself, under either dereplicate mode;
                       //  kept so that the function is whole on its own)
        const CandView none = {};   // not looked at
        emit_op(E, none, false, 0, -1, SMX_R_UNKNOWN, -1, -1, 0);
        return;
    }
    if (c.derep == SMX_DEREP_NONE) {   // demultiplex.py:181-197
        FOR_BEST_CANDS(c, ori, best, {
            if (best == 5) {   // resolve_specimen full branch (:555-575): specimens_for_barcodes_and_primers
                int first = -1, cnt = 0;
                for (int i = next_tied(c, v.h1, 0); i >= 0; i = next_tied(c, v.h1, i + 1))
                    for (int j = next_tied(c, v.h2, 0); j >= 0; j = next_tied(c, v.h2, j + 1)) {
                        int g1 = global_bc(c, v.h1, i), g2 = global_bc(c, v.h2, j);
                        specimens_for(P, g1, g2, v.f, v.r, first, cnt);
                    }
                if (cnt > 1) emit_op(E, v, true, cand_id, first, SMX_R_MULTIPLE, P->specrec[first].pool, -1, 0);
                else if (cnt == 1) emit_op(E, v, true, cand_id, first, SMX_R_FULL, P->specrec[first].pool, -1, 0);
                else emit_op(E, v, true, cand_id, -1, SMX_R_UNKNOWN, cand_pool, -1, SMX_OPF_NO_SPECIMEN);
            } else {
                emit_partial_or_unknown(E, v, cand_id, cand_pool);
            }
        })
        return;
    }
    // ---- dereplicate_matches (demultiplex.py:262-393); the best list is homogeneous in score
    if (best == 5) {
        // expanded entries in order: (candidate, tied b1, tied b2) -> specimen, or one None entry per
        // candidate without any specimen.  Groups keep first-appearance order (dict insertion).
        bool none_done = false;
        FOR_BEST_CANDS(c, ori, best, {
            bool any = false;
            for (int i = next_tied(c, v.h1, 0); i >= 0; i = next_tied(c, v.h1, i + 1))
                for (int j = next_tied(c, v.h2, 0); j >= 0; j = next_tied(c, v.h2, j + 1)) {
                    int spec = specimen_exact(P, global_bc(c, v.h1, i), global_bc(c, v.h2, j), v.f, v.r);
                    if (spec < 0) continue;
                    any = true;
                    // first appearance of this specimen? (earlier candidate, or earlier combo of this one)
                    bool seen = false;
                    {
                        const int cur_id = cand_id; const int ci = i; const int cj = j;
                        FOR_BEST_CANDS(c, ori, best, {
                            if (seen || cand_id > cur_id) continue;
                            if (cand_id < cur_id) { if (cand_has_specimen(c, v, spec)) seen = true; continue; }
                            for (int i2 = next_tied(c, v.h1, 0); i2 >= 0 && !seen; i2 = next_tied(c, v.h1, i2 + 1))
                                for (int j2 = next_tied(c, v.h2, 0); j2 >= 0; j2 = next_tied(c, v.h2, j2 + 1)) {
                                    if (i2 > ci || (i2 == ci && j2 >= cj)) break;
                                    if (specimen_exact(P, global_bc(c, v.h1, i2), global_bc(c, v.h2, j2), v.f, v.r) == spec) { seen = true; break; }
                                }
                        })
                    }
                    if (seen) continue;
                    // the group's winner: stable min of (b1d+b2d, p1d+p2d, file index sum) over its entries
                    int wkey = 0x7FFFFFFF, wid = -1;
                    FOR_BEST_CANDS(c, ori, best, {
                        int k = key_full(c.LP, v);
                        if (k < wkey && cand_has_specimen(c, v, spec)) { wkey = k; wid = cand_id; }
                    })
                    CandView w = cand_view(c, wid >> 1, wid & 1);
                    emit_op(E, w, true, wid, spec, SMX_R_DEREP_FULL, P->specrec[spec].pool, -1, 0);
                }
            if (!any && !none_done) {
                // the None group sits where its first entry appeared; it holds every best candidate
                // without a specimen ("other_matches", :361-363) -> resolve_specimen -> UNKNOWN (Q10)
                none_done = true;
                const int first_id = cand_id;
                FOR_BEST_CANDS(c, ori, best, {
                    if (cand_id < first_id) continue;
                    if (!cand_has_specimen(c, v, -1))
                        emit_op(E, v, true, cand_id, -1, SMX_R_UNKNOWN, cand_pool, -1, SMX_OPF_NO_SPECIMEN);
                })
            }
        })
        return;
    }
    if (best >= 3) {
        // dereplicate_partial_matches (:396-477): groups keyed (direction, barcode) for every tied barcode
        FOR_BEST_CANDS(c, ori, best, {
            bool fwd = v.b1;
            int h = fwd ? v.h1 : v.h2;
            for (int i = next_tied(c, h, 0); i >= 0; i = next_tied(c, h, i + 1)) {
                int gb = global_bc(c, h, i);
                const int cur_id = cand_id;
                bool seen = false;
                int wkey = 0x7FFFFFFF, wid = -1;
                FOR_BEST_CANDS(c, ori, best, {
                    if (v.b1 != fwd) continue;
                    int h2 = fwd ? v.h1 : v.h2;
                    if (!tied_has_global(c, h2, gb)) continue;
                    if (cand_id < cur_id) seen = true;
                    int k = key_partial(c.LP, v, fwd);
                    if (k < wkey) { wkey = k; wid = cand_id; }
                })
                if (seen) continue;
                CandView w = cand_view(c, wid >> 1, wid & 1);
                emit_partial_or_unknown(E, w, wid, c.LP.pair_pool[wid >> 1]);
            }
        })
        return;
    }
    // dereplicate_unknown_matches (:480-538): one stable minimum
    {
        int wkey = 0x7FFFFFFF, wid = -1;
        FOR_BEST_CANDS(c, ori, best, {
            int k = key_unknown(c.LP, v);
            if (k < wkey) { wkey = k; wid = cand_id; }
        })
        CandView w = cand_view(c, wid >> 1, wid & 1);
        emit_op(E, w, true, wid, -1, SMX_R_UNKNOWN, c.LP.pair_pool[wid >> 1], -1, 0);
    }
}

}  // namespace smx
#endif
