// smx_hits.hip -- the identify hot path: HW (infix) edit distances of every consensus of a job against every record of
// a reference set, the shorter sequence of each pair as the pattern, reduced on the device to the K best records per
// consensus.
//
// The layout is specimine's (smx_mine.hip): one chunk = one pattern x up to MINE_THREADS texts, one text per lane; the
// workgroup builds the pattern's Peq table in LDS (mine_build_peq) and every lane runs mine_pair (smx_mine_core.h) as it
// is.  What differs is where the texts come from and where the result goes: a work record (smx_hits_plan.h) names a
// window of an order array, so that a lane's text is ord[first + c * MINE_THREADS + lane], and a hit goes into the K
// slots of the pair's query by hits_insert (smx_hits_core.h), whichever of the two the pattern was.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_internal.h"
#include "smx_hits_core.h"
#include "smx_mine_lds.h"   // the chunk walk, mine_build_peq

namespace smx {

struct HitsAtomicMin {
    __device__ u64 operator()(u64 *p, u64 v) const { return atomicMin(p, v); }
};

// Workgroup b takes the contiguous chunks [b * per_block, (b + 1) * per_block) of the record list, record p owning
// chunks [chunk_start[p], chunk_start[p + 1]); the Peq table is rebuilt only when the pattern changes.
//   DIST = false (hits): a lane with d >= 0 packs the key and inserts it into keys[(job.row_off + q - q0) * K ..), which
//     the caller filled with 0xFF bytes.  On side Q the query is the workgroup's pattern and the target the lane's text;
//     on side T the query is the lane's text and the target the pattern.  A lane with d = -1 touches no global memory.
//   DIST = true (distances): d goes to dist[job.dist_off + (q - q0) * nt + t - t0], which the caller filled with -1.
template <int WR, bool DIST>
__global__ __launch_bounds__(MINE_THREADS) void hits_kernel(const unsigned char *__restrict__ bytes,
                                                            const uint64_t *__restrict__ off,
                                                            const int32_t *__restrict__ len,
                                                            const int32_t *__restrict__ klim,
                                                            const uint32_t *__restrict__ ord,
                                                            const HitsRec *__restrict__ recs,
                                                            const uint64_t *__restrict__ chunk_start, uint32_t n_recs,
                                                            const HitsJobDev *__restrict__ jobs, uint64_t per_block, int K,
                                                            u64 *keys, int32_t *dist, u64 *scratch, int scratch_words) {
    extern __shared__ u64 lds[];
    const ChunkLds L = chunk_lds(lds);
    const ChunkSpan S = chunk_span(chunk_start, n_recs, per_block);
    uint32_t p = chunk_owner(chunk_start, n_recs, S.lo);      // the record whose chunk range holds the first chunk
    uint32_t cur = 0xffffffffu;
    const unsigned lane = threadIdx.x;
    for (uint64_t v = S.lo; v < S.hi; v++) {
        while (chunk_start[p + 1] <= v) p++;
        const HitsRec R = recs[p];
        const HitsJobDev J = jobs[R.job];
        const uint32_t c = (uint32_t)(v - chunk_start[p]) * MINE_THREADS + lane;   // the text within the window
        const int m = len[R.pattern];
        const int W = (m + 63) >> 6, Wp = W | 1;
        if (R.pattern != cur) {
            __syncthreads();                       // the previous pattern's lanes are done with the table
            mine_build_peq(bytes + off[R.pattern], m, W, Wp, L.peq, L.rowmap, L.present);
            cur = R.pattern;
        }
        if (c < R.n) {
            const uint32_t text = ord[R.first + c];
            const int d = chunk_lane_state<WR>(scratch, scratch_words, [&](auto &st) {
                return mine_pair<WR>(st, L.peq, L.rowmap, m, W, Wp, klim[R.pattern], bytes + off[text], len[text]);
            });
            const uint32_t q = (R.side ? text : R.pattern) - J.q0, t = (R.side ? R.pattern : text) - J.t0;
            if constexpr (DIST) dist[J.dist_off + (uint64_t)q * J.nt + t] = d;
            else if (d >= 0) hits_insert(keys + (J.row_off + q) * (uint64_t)K, K, hits_key(d, m, t), HitsAtomicMin());
        }
    }
}

}  // namespace smx

extern "C" int smx_launch_hits(void *stream, int wr, int dist, const unsigned char *d_bytes, const uint64_t *d_off,
                               const int32_t *d_len, const int32_t *d_k, const uint32_t *d_ord, const void *d_recs,
                               const uint64_t *d_chunk_start, uint32_t n_recs, const void *d_jobs, int grid,
                               uint64_t per_block, size_t lds_bytes, int K, unsigned long long *d_keys, int32_t *d_dist,
                               unsigned long long *d_scratch, int scratch_words) {
    using namespace smx;
    if (K < 1 || K > HITS_MAX_K) return (int)hipErrorInvalidValue;
    // in the order of hits_kernel's parameters; every pointer is passed as the pointer it is
    void *args[] = {&d_bytes, &d_off, &d_len, &d_k, &d_ord, &d_recs, &d_chunk_start, &n_recs, &d_jobs, &per_block, &K,
                    &d_keys, &d_dist, &d_scratch, &scratch_words};
    auto pick = [&](auto WR) { return dist ? (const void *)hits_kernel<WR(), true> : (const void *)hits_kernel<WR(), false>; };
    return chunk_launch(stream, wr, pick, n_recs, grid, per_block, lds_bytes, args);
}
