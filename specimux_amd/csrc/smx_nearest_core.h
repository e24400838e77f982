// smx_nearest_core.h -- what the crosstalk kernel (smx_nearest.hip) adds to the per-pair code of clusters
// (smx_pairs_core.h pairs_pair, unchanged): the records of a call, the 64-bit key of a (distance, ref) offer, the
// own / other choice and the limit of a pair.
//
// The key.  A pair within its limit offers ((uint64)d << 32) | ref, ref being the ref's index in the sequence array;
// a read keeps the minimum of the offers of its own group and the minimum of all others.  Keys of distinct refs are
// distinct and unsigned order on them is "smaller distance, then lower ref index", a total order: the minimum of a set
// of offers does not depend on the order in which lanes, runs, classes or launches make them.  No offer is UINT64_MAX
// (d <= INT32_MAX), which therefore says "no ref within the limit".
//
// Host/device code like smx_pairs_core.h: the kernel and tests/cpu/nearest_host.h run the same lines.
#ifndef SMX_NEAREST_CORE_H
#define SMX_NEAREST_CORE_H
#include "smx_pairs_core.h"

namespace smx {

constexpr u64 NEAREST_NONE = ~0ull;

struct NearestJobDev {   // one smx_nearest_job with its output offsets
    uint32_t q0, nq, t0, nt;
    uint64_t best_off;   // its nt entries of best_own / best_other
    uint64_t dist_off;   // its nq x nt distances (distances mode)
};

struct NearestRun {      // consecutive refs of one state class x the reads of one job: ceil(nt / MINE_THREADS) chunks
    uint32_t job;        // index into the NearestJobDev array
    uint32_t first, n;   // refs [first, first + n) of the class's ref list
};

struct NearestKeys {     // a lane's running minima over one run
    u64 own = NEAREST_NONE, other = NEAREST_NONE;
};

SMX_MINE_HD inline u64 nearest_key(int d, uint32_t ref) { return ((u64)(uint32_t)d << 32) | ref; }

// the limit of a (ref, read) pair: the smx_pairs_* rule
SMX_MINE_HD inline int nearest_limit(int k_ref, int k_read) { return (k_ref < 0 || k_read < 0) ? -1 : (k_ref > k_read ? k_ref : k_read); }

// a pair's distance d (-1: above the limit, no offer) to the lane's keys
SMX_MINE_HD inline void nearest_offer(NearestKeys &K, bool same_group, int d, uint32_t ref) {
    if (d < 0) return;
    const u64 key = nearest_key(d, ref);
    u64 &slot = same_group ? K.own : K.other;
    if (key < slot) slot = key;
}

}  // namespace smx

#endif  // SMX_NEAREST_CORE_H
