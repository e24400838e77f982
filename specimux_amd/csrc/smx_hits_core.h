// smx_hits_core.h -- what the identify kernel (smx_hits.hip) adds to the per-pair code of specimine (smx_mine_core.h
// mine_pair, unchanged): the records of a call, the pair rule, the 64-bit key of a hit and the top-K insertion
// (DESIGN.md §17).
//
// The pair rule.  Of a (query, target) pair the shorter sequence is the pattern and the other the text, the query at
// equal length; d = HW(pattern in text) under the limit k[pattern].  The pair is eligible only if
// len(pattern) * 1000 >= min_cov_permille * len(text).
//
// The key.  A hit offers (ppm << 43) | (d << 24) | (t - t0) with ppm = (d << 20) / len(pattern) (integer division,
// <= 2^20), d < 2^19 and the target's index within the job < 2^24.  Unsigned order on keys is "lower edit fraction,
// then fewer edits, then lower target index", a total order in which keys of distinct targets differ.  No key is
// UINT64_MAX (ppm <= 2^20 < 2^21 - 1), which therefore says "empty slot".
//
// Host/device code like smx_nearest_core.h: the kernel and tests/cpu/hits_host.h run the same lines.
#ifndef SMX_HITS_CORE_H
#define SMX_HITS_CORE_H
#include "smx_mine_core.h"

namespace smx {

constexpr u64 HITS_NONE = ~0ull;
constexpr int HITS_MAX_K = 16;                     // SMX_HITS_MAX_K of include/smx.h
constexpr int64_t HITS_MAX_PATTERN = 1ll << 19;    // a pattern is shorter than this: d fits 19 bits
constexpr uint64_t HITS_MAX_TARGETS = 1ull << 24;  // targets of one job: the index fits 24 bits

struct HitsJobDev {      // one smx_hits_job with its output offsets
    uint32_t q0, nq, t0, nt;
    uint64_t row_off;    // its first query's row of K keys: sum of the earlier jobs' nq
    uint64_t dist_off;   // its nq x nt distances (distances mode)
};

struct HitsRec {         // one pattern x a window of its job's order array: ceil(n / MINE_THREADS) chunks
    uint32_t job;        // index into the HitsJobDev array
    uint32_t side;       // 0 = side Q: the pattern is a query, the texts are targets; 1 = side T: the other way round
    uint32_t pattern;    // the pattern's index in the sequence array
    uint32_t first, n;   // the texts are ord[first .. first + n)
};

// len(pattern) * 1000 >= min_cov_permille * len(text), in 64 bits
SMX_MINE_HD inline bool hits_eligible(int len_pattern, int len_text, int min_cov_permille) {
    return (int64_t)len_pattern * 1000 >= (int64_t)min_cov_permille * len_text;
}

// the longest text a pattern of m bytes is eligible with (int64: no bound at coverage 0)
SMX_MINE_HD inline int64_t hits_max_text(int m, int min_cov_permille) {
    return min_cov_permille <= 0 ? INT64_MAX : (int64_t)m * 1000 / min_cov_permille;
}

// the key of a hit: d edits of a pattern of m bytes (0 <= d <= m < 2^19), target index within the job < 2^24
SMX_MINE_HD inline u64 hits_key(int d, int m, uint32_t target_in_job) {
    const u64 ppm = ((u64)(uint32_t)d << 20) / (u64)(uint32_t)m;
    return (ppm << 43) | ((u64)(uint32_t)d << 24) | (u64)target_in_job;
}

SMX_MINE_HD inline uint32_t hits_key_ppm(u64 key) { return (uint32_t)(key >> 43); }
SMX_MINE_HD inline uint32_t hits_key_d(u64 key) { return (uint32_t)(key >> 24) & 0x7ffffu; }
SMX_MINE_HD inline uint32_t hits_key_target(u64 key) { return (uint32_t)key & 0xffffffu; }

// Offer `key` to a query's K slots (ascending, HITS_NONE = empty).  amin(p, v) is an atomic minimum that returns the
// old value: atomicMin on the device, a plain function in the simulation.  Each atomic leaves {slot, carried} =
// {min, max} of {old slot, offered}, so the multiset pushed on to slot s + 1 is the multiset offered to slot s minus
// its minimum, whatever the interleaving: slot s ends as the (s + 1)-th smallest key offered.  Slot values only fall,
// so a key above the slots[K - 1] read here (by a plain load, possibly stale) is above the final one as well.
template <typename AtomicMin>
SMX_MINE_HD inline void hits_insert(u64 *slots, int K, u64 key, AtomicMin amin) {
    if (key > slots[K - 1]) return;
    for (int s = 0; s < K; s++) {
        const u64 old = amin(&slots[s], key);
        key = old > key ? old : key;
        if (key == HITS_NONE) return;
    }
}

}  // namespace smx

#endif  // SMX_HITS_CORE_H
