// smx_reach_core.h -- the per-pair code of the bimera kernel (smx_reach.hip): how far a query prefix runs within e edits
// of a parent, for every e in 0..E, by furthest-reaching diagonals (Landau-Vishkin).
//
// D(i, j) is the unit-cost edit distance of q[0:i] and r[0:j], anchored at both starts.  Diagonal d holds the cells
// (i, i + d); along a diagonal D never falls, so "the furthest point of diagonal d within e edits" is one number
// fr_e[d] = max { i : D(i, i + d) <= e }, and
//   fr_0[0]  = the common prefix of q and r, every other diagonal empty (REACH_NEG)
//   fr_e[d]  = slide(min(max(fr_{e-1}[d] + 1, fr_{e-1}[d - 1], fr_{e-1}[d + 1] + 1), n, m - d))
// where slide follows equal bytes down the diagonal.  The minimum is the clamp to the matrix: a candidate one past the
// end of either sequence falls back along its diagonal to the last cell, whose distance is at most one more than its
// neighbour's (a point stuck at a sequence's end stays where it is).  Diagonals outside -n..m hold no cell and stay
// empty.  reach(q, r, e) = max over d of fr_e[d].
//
// The key of an offer is ((0xFFFFFFFF - reach) << 32) | t with t the target's index in the call's sequence array:
// unsigned order is "longer reach, then lower index", keys of distinct targets differ, and no key is UINT64_MAX
// (t < n_seqs <= 2^32 - 1), which therefore says "empty slot".  Offers go into two slots by hits_insert
// (smx_hits_core.h).
//
// Host/device code like smx_hits_core.h: the kernel and tests/cpu/reach_host.h run the same lines; the kernel keeps
// fr of diagonal lane - E in a register and takes its neighbours' by shuffles, the host loop keeps an array.
#ifndef SMX_REACH_CORE_H
#define SMX_REACH_CORE_H
#include "smx_hits_core.h"

namespace smx {

constexpr int REACH_MAX_E = 15;                    // SMX_REACH_MAX_E of include/smx.h: 2 E + 1 diagonals fit 32 lanes
constexpr int REACH_LANES = 32;                    // lanes of one (pair, side): half a wave
constexpr int REACH_SLOTS = 2;                     // keys kept per (query, side, e)
constexpr int REACH_NEG = -(1 << 30);              // an empty diagonal
constexpr int64_t REACH_MAX_LEN = (1 << 30) - 1;   // a sequence is at most this long: i + d and fr + 1 stay in an int
constexpr uint32_t REACH_CHUNK = 64;               // targets of one chunk: 128 (pair, side) items over the workgroup's 4 groups
constexpr uint32_t REACH_NOT_ELIGIBLE = 0xffffffffu;

struct ReachJobDev {     // one smx_reach_job with its output offsets
    uint32_t q0, nq, t0, nt;
    uint64_t row_off;    // its first query's row: sum of the earlier jobs' nq
    uint64_t mat_off;    // its first pair (matrix mode): sum of the earlier jobs' nq x nt
};

struct ReachRec {        // one query x its job's targets: ceil(nt / REACH_CHUNK) chunks
    uint32_t job;        // index into the ReachJobDev array
    uint32_t query;      // the query's index in the sequence array
};

SMX_MINE_HD inline int reach_min(int a, int b) { return a < b ? a : b; }
SMX_MINE_HD inline int reach_max(int a, int b) { return a > b ? a : b; }

// 8 bytes from any address
SMX_MINE_HD inline u64 reach_load8(const unsigned char *p) {
    u64 x;
    __builtin_memcpy(&x, p, 8);
    return x;
}

// From (i, j), both inside the matrix, follow equal bytes: the new i.  8 bytes at a time; the run is bounded by what is
// left of BOTH sequences, since what lies behind a sequence's end (padding, the next sequence) may well compare equal.
// Reads at most 7 bytes past the end of either sequence.
SMX_MINE_HD inline int reach_slide(const unsigned char *q, int n, const unsigned char *r, int m, int i, int j) {
    const int room = reach_min(n - i, m - j);
    int run = 0;
    while (run < room) {
        const u64 x = reach_load8(q + i + run) ^ reach_load8(r + j + run);
        if (x) {
            run += __builtin_ctzll(x) >> 3;
            break;
        }
        run += 8;
    }
    return i + reach_min(run, room);
}

// fr_e[d] before the slide from fr_{e-1} of d (own), d - 1 (below) and d + 1 (above); REACH_NEG if the diagonal is
// outside the matrix or no predecessor holds a point.
SMX_MINE_HD inline int reach_step(int own, int below, int above, int d, int n, int m) {
    if (d < -n || d > m) return REACH_NEG;
    const int cand = reach_max(own + 1, reach_max(below, above + 1));
    if (cand < 0) return REACH_NEG;
    return reach_min(cand, reach_min(n, m - d));
}

SMX_MINE_HD inline u64 reach_key(uint32_t reach, uint32_t t) { return ((u64)(0xffffffffu - reach) << 32) | (u64)t; }
SMX_MINE_HD inline uint32_t reach_key_reach(u64 key) { return 0xffffffffu - (uint32_t)(key >> 32); }
SMX_MINE_HD inline uint32_t reach_key_target(u64 key) { return (uint32_t)key; }

// target t counts for query q
SMX_MINE_HD inline bool reach_eligible(uint32_t q, uint32_t t, uint32_t need_q, uint32_t weight_t) {
    return t != q && weight_t >= need_q;
}

// where the results of (row or pair, side, e) lie: REACH_SLOTS keys per (query row, side, e); one value per (pair, side, e)
SMX_MINE_HD inline uint64_t reach_slot_at(uint64_t row, int side, int e, int E) {
    return ((row * 2 + (uint64_t)side) * (uint64_t)(E + 1) + (uint64_t)e) * REACH_SLOTS;
}
SMX_MINE_HD inline uint64_t reach_value_at(uint64_t pair, int side, int e, int E) {
    return (pair * 2 + (uint64_t)side) * (uint64_t)(E + 1) + (uint64_t)e;
}

}  // namespace smx

#endif  // SMX_REACH_CORE_H
