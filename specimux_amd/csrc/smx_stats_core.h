// smx_stats_core.h -- the per-read logic of the match statistics (specimux-stats), host/device.
//
// One read = the hit table row the demux kernel dumped for it (smx_hit per (primer, end)) + its primary record.
// stats_read() rebuilds from those the rows the reference's trace_stats.py would build from the read's trace events
// (one per PRIMER_MATCHED event, or one synthesised row for a read without a candidate), packs each row into a
// 64-bit key (layout: include/smx.h, "Match statistics") and hands it to a sink.  stats_find_slot() is the
// open-addressing (key, count) table both the kernel (LDS and global) and the CPU simulation count into.
// Shared by smx_stats.hip and tests/cpu/stats_sim.cpp, which runs this code without a GPU.
#ifndef SMX_STATS_CORE_H
#define SMX_STATS_CORE_H
#include <stdint.h>
#include "smx.h"
#include "smx_hd.h"

namespace smx {

#define SMX_STATS_EMPTY (~0ull)
// shape of the kernel's on-chip combine (smx_stats.hip); the CPU simulation walks the reads in the same workgroup chunks
#define STATS_THREADS 256
#ifndef STATS_LCAP               // (the simulation is also built with a tiny table, to drive rows past it)
#define STATS_LCAP 2048          // LDS table of a workgroup: 16 KiB of keys + 8 KiB of 32-bit counts
#define STATS_LPROBE 16          // probes before a row bypasses the LDS table
#endif
#define STATS_GPROBE_MAX 8192u   // a probe run this long in the global table counts as a full table

struct StatsPanel {        // what the rule needs of the panel; pointers are device pointers in the kernel
    int NP, NPAIR, preorient;
    const int *pdir;       // per primer: 0 forward, 1 reverse
    const int *pair_f, *pair_r;
};

// outcome / resolution class of a row (SMX_STATS_CLASS_* in smx.h)
SMX_HD unsigned stats_class_of_rtype(unsigned rtype) {
    switch (rtype) {
        case SMX_R_FULL: return SMX_STATS_CLASS_FULL;
        case SMX_R_PARTIAL_FWD: return SMX_STATS_CLASS_PARTIAL_FWD;
        case SMX_R_PARTIAL_REV: return SMX_STATS_CLASS_PARTIAL_REV;
        case SMX_R_MULTIPLE: return SMX_STATS_CLASS_MULTIPLE;
        default: return SMX_STATS_CLASS_UNKNOWN;   // UNKNOWN, and DEREP_FULL: the reference logs no SPECIMEN_RESOLVED for it
    }
}

SMX_HD uint64_t stats_key(unsigned ori, unsigned pair1, unsigned p1, unsigned p2, unsigned b1, unsigned b2, unsigned cls,
                          unsigned first) {
    return (uint64_t)ori | ((uint64_t)pair1 << SMX_STATS_PAIR_SHIFT) | ((uint64_t)p1 << SMX_STATS_P1_SHIFT) |
           ((uint64_t)p2 << SMX_STATS_P2_SHIFT) | ((uint64_t)b1 << SMX_STATS_B1_SHIFT) | ((uint64_t)b2 << SMX_STATS_B2_SHIFT) |
           ((uint64_t)cls << SMX_STATS_CLASS_SHIFT) | ((uint64_t)first << SMX_STATS_FIRST_SHIFT);
}

// the two ends of candidate (pair, o): forward primer's hit h1, reverse primer's hit h2
struct StatsCand {
    bool p1, p2, b1, b2;
    int bc1, bc2;
    SMX_HD bool exists() const { return p1 || p2; }
    SMX_HD int score() const {   // reference demultiplex.py:226-236
        if (p1 && p2 && b1 && b2) return 5;
        if (p1 && p2 && (b1 || b2)) return 4;
        if ((p1 || p2) && (b1 || b2)) return 3;
        if (p1 && p2) return 2;
        return (p1 || p2) ? 1 : 0;
    }
};

SMX_HD StatsCand stats_cand(const smx_hit *hits, int f, int r, int o) {
    const smx_hit &h1 = hits[2 * f + o], &h2 = hits[2 * r + (1 - o)];
    StatsCand c;
    c.p1 = h1.pdist >= 0;
    c.p2 = h2.pdist >= 0;
    c.b1 = c.p1 && h1.bbest >= 0;
    c.b2 = c.p2 && h2.bbest >= 0;
    c.bc1 = c.b1 ? h1.first_tied : -1;
    c.bc2 = c.b2 ? h2.first_tied : -1;
    return c;
}

// determine_orientation from the vote bits: 0 unknown, 1 forward, 2 reverse
SMX_HD unsigned stats_orientation(const StatsPanel &P, const smx_hit *hits) {
    if (!P.preorient) return 0;
    int f = 0, r = 0;
    for (int p = 0; p < P.NP; p++) {
        const int va = hits[2 * p].flags & 1, vb = hits[2 * p + 1].flags & 1;
        if (P.pdir[p] == 0) { f += va; r += vb; } else { f += vb; r += va; }
    }
    return (f > 0 && r == 0) ? 1u : (r > 0 && f == 0) ? 2u : 0u;
}

struct StatsReadInfo {     // what the simulation's coverage counters and the kernel's fallback list need
    int n_cand, n_discarded;
    bool fallback;         // the primary record is a trim-to-empty fallback: the host decides this read
};

// Rows of one read.  `hits` = the read's 2 * NP hit records, `op` = its primary record.  sink(key) once per row.
template <class Sink>
SMX_HD StatsReadInfo stats_read(const StatsPanel &P, const smx_hit *hits, const smx_op &op, Sink &&sink) {
    StatsReadInfo info = {0, 0, false};
    if (op.rtype == SMX_R_FILTERED) {
        sink(stats_key(0, 0, 0, 0, 0, 0, SMX_STATS_CLASS_UNKNOWN, 1));
        return info;
    }
    if (op.flags & SMX_OPF_TRIM_EMPTY) {
        info.fallback = true;
        return info;
    }
    const unsigned ori = stats_orientation(P, hits);
    int best = 0;
    for (int pr = 0; pr < P.NPAIR; pr++)
        for (int o = 0; o < 2; o++) {
            if ((o == 0 && ori == 2) || (o == 1 && ori == 1)) continue;
            const StatsCand c = stats_cand(hits, P.pair_f[pr], P.pair_r[pr], o);
            if (!c.exists()) continue;
            const int s = c.score();
            best = s > best ? s : best;
            info.n_cand++;
        }
    if (info.n_cand == 0) {
        sink(stats_key(ori, 0, 0, 0, 0, 0, SMX_STATS_CLASS_UNKNOWN, 1));
        return info;
    }
    const unsigned cls = stats_class_of_rtype(op.rtype);
    unsigned first = 1;
    for (int pr = 0; pr < P.NPAIR; pr++)
        for (int o = 0; o < 2; o++) {
            if ((o == 0 && ori == 2) || (o == 1 && ori == 1)) continue;
            const StatsCand c = stats_cand(hits, P.pair_f[pr], P.pair_r[pr], o);
            if (!c.exists()) continue;
            const bool discarded = c.score() < best;
            info.n_discarded += discarded ? 1 : 0;
            sink(stats_key(ori, (unsigned)pr + 1, c.p1, c.p2, (unsigned)(c.bc1 + 1), (unsigned)(c.bc2 + 1),
                           discarded ? (unsigned)SMX_STATS_CLASS_DISCARDED : cls, first));
            first = 0;
        }
    return info;
}

SMX_HD uint32_t stats_hash(uint64_t key) {
    key ^= key >> 29;
    key *= 0x9E3779B97F4A7C15ull;
    return (uint32_t)(key >> 32);
}

// claim-or-find: the value that was in *slot before (SMX_STATS_EMPTY: this call claimed it)
SMX_HD uint64_t stats_claim(uint64_t *slot, uint64_t key) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)atomicCAS((unsigned long long *)slot, (unsigned long long)SMX_STATS_EMPTY, (unsigned long long)key);
#else
    const uint64_t old = *slot;
    if (old == SMX_STATS_EMPTY) *slot = key;
    return old;
#endif
}

// Slot of `key` in an open-addressing table of `cap` (a power of two) keys, linear probing, at most max_probe probes;
// -1 when every probed slot belongs to another key (the table, or this stretch of it, is full).
SMX_HD int stats_find_slot(uint64_t *keys, uint32_t cap, uint64_t key, uint32_t max_probe) {
    uint32_t s = stats_hash(key) & (cap - 1);
    for (uint32_t i = 0; i < max_probe; i++) {
        uint64_t k = keys[s];
        if (k == SMX_STATS_EMPTY) k = stats_claim(&keys[s], key);
        if (k == SMX_STATS_EMPTY || k == key) return (int)s;
        s = (s + 1) & (cap - 1);
    }
    return -1;
}

}  // namespace smx
#endif
