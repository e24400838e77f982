// smx_reach.hip -- the bimera hot path: for every query of a job and every eligible target, how far a prefix of the
// query (side 0) and a suffix (side 1) run within e edits of the target, e = 0..E, reduced on the device to the two
// furthest-reaching targets per (query, side, e).
//
// Unlike the other long-read kernels this one builds no Peq table and scans no column: it is a diagonal wavefront
// (Landau-Vishkin).  One (pair, side) belongs to half a wave of 32 lanes, lane l holding the furthest point of diagonal
// l - E in a register (2 E + 1 <= 31 diagonals).  A step takes the three predecessors from the neighbouring lanes by
// shuffles of width 32 (reach_step), slides 8 bytes at a time (reach_slide) and takes the group's maximum; lane e keeps
// reach(e) and offers its key at the end.  The right side runs the same code over the reversed copies that the host
// uploads behind the forward ones.
//
// The work list is the chunked kernels' (smx_mine_lds.h chunk_span / chunk_owner): a record is one (job, query), a chunk
// REACH_CHUNK targets of its job x 2 sides, and the workgroup's four groups take the chunk's items in turn.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_internal.h"
#include "smx_reach_core.h"
#include "smx_mine_lds.h"   // the chunk walk

namespace smx {

struct ReachAtomicMin {
    __device__ u64 operator()(u64 *p, u64 v) const { return atomicMin(p, v); }
};

__device__ __forceinline__ int reach_group_max(int x) {
    for (int s = REACH_LANES / 2; s; s >>= 1) x = max(x, __shfl_xor(x, s, REACH_LANES));
    return x;
}

// bytes / doff: the padded sequences, forwards at [0, n_seqs) and reversed at [n_seqs, 2 n_seqs); len / weight / need
// per sequence.  MATRIX = false: lane e offers reach_key(reach(e), t) to the query's slots in keys, which the caller
// filled with 0xFF bytes.  MATRIX = true: lane e writes reach(e) to values, which the caller filled with 0xFF bytes.
// A pair that is not eligible touches no output.
template <bool MATRIX>
__global__ __launch_bounds__(MINE_THREADS) void reach_kernel(const unsigned char *__restrict__ bytes,
                                                             const uint64_t *__restrict__ doff,
                                                             const int32_t *__restrict__ len,
                                                             const uint32_t *__restrict__ weight,
                                                             const uint32_t *__restrict__ need,
                                                             const ReachRec *__restrict__ recs,
                                                             const uint64_t *__restrict__ chunk_start, uint32_t n_recs,
                                                             const ReachJobDev *__restrict__ jobs, uint64_t per_block,
                                                             int E, uint32_t n_seqs, u64 *keys, uint32_t *values) {
    const ChunkSpan S = chunk_span(chunk_start, n_recs, per_block);
    uint32_t p = chunk_owner(chunk_start, n_recs, S.lo);      // the record whose chunk range holds the first chunk
    const unsigned group = threadIdx.x / REACH_LANES, lane = threadIdx.x % REACH_LANES;
    const int d = (int)lane - E;
    for (uint64_t v = S.lo; v < S.hi; v++) {
        while (chunk_start[p + 1] <= v) p++;
        const ReachRec R = recs[p];
        const ReachJobDev J = jobs[R.job];
        const uint32_t q = R.query, first = (uint32_t)(v - chunk_start[p]) * REACH_CHUNK;
        const uint32_t count = min(REACH_CHUNK, J.nt - first);
        const int n = len[q];
        const uint32_t need_q = need[q];
        // an item is (target, side); the four groups of the workgroup take them in turn.  Everything up to the shuffles
        // is uniform within a group
        for (uint32_t item = group; item < count * 2; item += MINE_THREADS / REACH_LANES) {
            const uint32_t ti = first + (item >> 1), t = J.t0 + ti;
            const int side = (int)(item & 1);
            if (!reach_eligible(q, t, need_q, weight[t])) continue;
            const unsigned char *qs = bytes + doff[(size_t)side * n_seqs + q], *rs = bytes + doff[(size_t)side * n_seqs + t];
            const int m = len[t];
            int fr = d == 0 ? reach_slide(qs, n, rs, m, 0, 0) : REACH_NEG;
            int best = reach_group_max(fr);
            int mine = best;                       // lane 0's; the others are set below
            int e = 1;
            for (; e <= E && best < n; e++) {
                int below = __shfl_up(fr, 1, REACH_LANES), above = __shfl_down(fr, 1, REACH_LANES);
                if (lane == 0) below = REACH_NEG;
                if (lane == REACH_LANES - 1) above = REACH_NEG;
                fr = reach_step(fr, below, above, d, n, m);
                if (fr >= 0) fr = reach_slide(qs, n, rs, m, fr, fr + d);
                best = reach_group_max(fr);
                if (lane == (unsigned)e) mine = best;
            }
            if (lane >= (unsigned)e) mine = best;  // the whole query was reached at step e - 1: it stays reached
            if (lane <= (unsigned)E) {
                if constexpr (MATRIX) {
                    values[reach_value_at(J.mat_off + (uint64_t)(q - J.q0) * J.nt + ti, side, (int)lane, E)] = (uint32_t)mine;
                } else {
                    hits_insert(keys + reach_slot_at(J.row_off + (q - J.q0), side, (int)lane, E), REACH_SLOTS,
                                reach_key((uint32_t)mine, t), ReachAtomicMin());
                }
            }
        }
    }
}

}  // namespace smx

extern "C" int smx_launch_reach(void *stream, int matrix, const unsigned char *d_bytes, const uint64_t *d_doff,
                                const int32_t *d_len, const uint32_t *d_weight, const uint32_t *d_need, const void *d_recs,
                                const uint64_t *d_chunk_start, uint32_t n_recs, const void *d_jobs, int grid,
                                uint64_t per_block, int E, uint32_t n_seqs, unsigned long long *d_keys, uint32_t *d_values) {
    using namespace smx;
    if (E < 0 || E > REACH_MAX_E || n_recs == 0 || grid < 1 || per_block < 1) return (int)hipErrorInvalidValue;
    // in the order of reach_kernel's parameters; every pointer is passed as the pointer it is
    void *args[] = {&d_bytes, &d_doff, &d_len, &d_weight, &d_need, &d_recs, &d_chunk_start, &n_recs, &d_jobs, &per_block,
                    &E, &n_seqs, &d_keys, &d_values};
    const void *fn = matrix ? (const void *)reach_kernel<true> : (const void *)reach_kernel<false>;
    return (int)hipLaunchKernel(fn, dim3(grid), dim3(MINE_THREADS), args, 0, (hipStream_t)stream);
}
