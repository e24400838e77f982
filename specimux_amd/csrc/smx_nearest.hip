// smx_nearest.hip -- the crosstalk hot path: NW (global) edit distances of every read of a job to every ref of the
// job, reduced on the device to the nearest ref of the read's own group and the nearest of all others.
//
// The layout is clusters' (smx_pairs.hip) turned rectangular: a ref is the query, its Peq table built in LDS
// (mine_build_peq), a read is the target, one per lane, and every lane runs pairs_pair (smx_pairs_core.h) as it is.
// One chunk = MINE_THREADS reads of a job x a run of consecutive refs of one state class (smx_nearest_plan.h): for each
// ref of the run the workgroup synchronises and rebuilds the table, then every lane aligns its read.  A lane keeps its
// two running keys (smx_nearest_core.h) in registers over the run and issues at most two 64-bit atomic minima at its
// end.  The limit of a pair is max(k[ref], k[read]), integers the host computed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_internal.h"
#include "smx_mine_lds.h"
#include "smx_nearest_core.h"

namespace smx {

// Workgroup b takes the contiguous chunks [b * per_block, (b + 1) * per_block) of the run list, run p owning chunks
// [chunk_start[p], chunk_start[p + 1]); chunk c of a run covers the job's reads [c * MINE_THREADS, (c + 1) * MINE_THREADS).
//   DIST = true (distances): every pair's d goes to dist[job.dist_off + (ref - q0) * nt + read - t0], plain stores.
//   DIST = false (nearest): atomicMin of the lane's keys into best_own / best_other[job.best_off + read - t0], which the
//     caller filled with 0xFF bytes; a lane without an offer writes nothing.
template <int WR, bool DIST>
__global__ __launch_bounds__(MINE_THREADS) void nearest_kernel(const unsigned char *__restrict__ bytes,
                                                               const uint64_t *__restrict__ off,
                                                               const int32_t *__restrict__ len,
                                                               const int32_t *__restrict__ klim,
                                                               const uint32_t *__restrict__ group,
                                                               const uint32_t *__restrict__ refs,
                                                               const NearestRun *__restrict__ runs,
                                                               const uint64_t *__restrict__ chunk_start, uint32_t n_runs,
                                                               const NearestJobDev *__restrict__ jobs, uint64_t per_block,
                                                               u64 *best_own, u64 *best_other, int32_t *dist,
                                                               u64 *scratch, int scratch_words) {
    extern __shared__ u64 lds[];
    const ChunkLds L = chunk_lds(lds);
    const ChunkSpan S = chunk_span(chunk_start, n_runs, per_block);
    uint32_t p = chunk_owner(chunk_start, n_runs, S.lo);      // the run whose chunk range holds the first chunk
    const unsigned lane = threadIdx.x;
    for (uint64_t v = S.lo; v < S.hi; v++) {
        while (chunk_start[p + 1] <= v) p++;
        const NearestRun R = runs[p];
        const NearestJobDev J = jobs[R.job];
        const uint32_t ti = (uint32_t)(v - chunk_start[p]) * MINE_THREADS + lane;   // the read within the job
        const bool active = ti < J.nt;
        const uint32_t t = J.t0 + (active ? ti : 0u);
        const int kt = klim[t], n = len[t];
        const uint32_t gt = group[t];
        const unsigned char *tb = bytes + off[t];
        NearestKeys K;
        for (uint32_t x = 0; x < R.n; x++) {
            const uint32_t ref = refs[R.first + x];
            const int m = len[ref];
            const int W = (m + 63) >> 6, Wp = W | 1;
            __syncthreads();                       // the previous ref's lanes are done with the table
            mine_build_peq(bytes + off[ref], m, W, Wp, L.peq, L.rowmap, L.present);
            if (active) {
                const int k = nearest_limit(klim[ref], kt);
                const int d = chunk_lane_state<WR>(scratch, scratch_words, [&](auto &st) {
                    return pairs_pair<WR>(st, L.peq, L.rowmap, m, W, Wp, k, tb, n);
                });
                if constexpr (DIST) dist[J.dist_off + (uint64_t)(ref - J.q0) * J.nt + ti] = d;
                else nearest_offer(K, group[ref] == gt, d, ref);
            }
        }
        if constexpr (!DIST) {
            if (active && K.own != NEAREST_NONE) atomicMin(best_own + J.best_off + ti, K.own);
            if (active && K.other != NEAREST_NONE) atomicMin(best_other + J.best_off + ti, K.other);
        }
    }
}

}  // namespace smx

extern "C" int smx_launch_nearest(void *stream, int wr, int dist, const unsigned char *d_bytes, const uint64_t *d_off,
                                  const int32_t *d_len, const int32_t *d_k, const uint32_t *d_group,
                                  const uint32_t *d_refs, const void *d_runs, const uint64_t *d_chunk_start,
                                  uint32_t n_runs, const void *d_jobs, int grid, uint64_t per_block, size_t lds_bytes,
                                  unsigned long long *d_best_own, unsigned long long *d_best_other, int32_t *d_dist,
                                  unsigned long long *d_scratch, int scratch_words) {
    using namespace smx;
    // in the order of nearest_kernel's parameters; every pointer is passed as the pointer it is
    void *args[] = {&d_bytes, &d_off, &d_len, &d_k, &d_group, &d_refs, &d_runs, &d_chunk_start, &n_runs, &d_jobs,
                    &per_block, &d_best_own, &d_best_other, &d_dist, &d_scratch, &scratch_words};
    auto pick = [&](auto WR) { return dist ? (const void *)nearest_kernel<WR(), true> : (const void *)nearest_kernel<WR(), false>; };
    return chunk_launch(stream, wr, pick, n_runs, grid, per_block, lds_bytes, args);
}
