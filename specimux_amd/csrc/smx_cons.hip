// smx_cons.hip -- the consensus hot path: every member read of a cluster aligned to the cluster's draft with traceback
// (cons_align_kernel), and the pileup rows reduced to per-position votes (cons_vote_kernel).  DESIGN.md §15.
//
// The alignment keeps the layout of smx_mine.hip / smx_pairs.hip: one chunk = one job's draft x up to MINE_THREADS member
// reads, one per lane; the workgroup builds the draft's Peq in LDS (mine_build_peq) and every lane runs cons_pair
// (smx_cons_core.h) over its own read: the forward pass leaves its history in the workgroup's slice of the history
// workspace, [column][block in band][lane], the walk back reads it and writes the lane's pileup row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_internal.h"
#include "smx_mine_lds.h"
#include "smx_cons_core.h"

namespace smx {

// Workgroup b takes the contiguous chunks [b * per_block, (b + 1) * per_block) of the job list, job p owning chunks
// [chunk_start[p], chunk_start[p + 1]).  Lane l of chunk c of a job handles member c * MINE_THREADS + l: its distance
// goes to dist[job.dist_off + member], its row (distance >= 0 only) to rows[job.rows_off + member * (m + 1) ...].
template <int WR>
__global__ __launch_bounds__(MINE_THREADS) void cons_align_kernel(const unsigned char *__restrict__ bytes,
                                                                  const uint64_t *__restrict__ off,
                                                                  const int32_t *__restrict__ len,
                                                                  const int32_t *__restrict__ klim,
                                                                  const ConsJobDev *__restrict__ jobs,
                                                                  const uint64_t *__restrict__ chunk_start, uint32_t n_jobs,
                                                                  uint64_t per_block, uint32_t *rows, int32_t *dist,
                                                                  cons_pm *hist_pm, int *hist_s, uint64_t hist_slice,
                                                                  u64 *scratch, int scratch_words) {
    extern __shared__ u64 lds[];
    const ChunkLds L = chunk_lds(lds);
    const ChunkSpan S = chunk_span(chunk_start, n_jobs, per_block);
    uint32_t p = chunk_owner(chunk_start, n_jobs, S.lo);      // the job whose chunk range holds the first chunk
    uint32_t cur_q = 0xffffffffu;
    const unsigned lane = threadIdx.x;
    // the workgroup's history slice: hist_slice entries per lane
    const size_t hbase = (size_t)blockIdx.x * hist_slice * MINE_THREADS + lane;
    for (uint64_t v = S.lo; v < S.hi; v++) {
        while (chunk_start[p + 1] <= v) p++;
        const ConsJobDev J = jobs[p];
        const int m = len[J.draft];
        const int W = (m + 63) >> 6, Wp = W | 1;
        if (J.draft != cur_q) {
            __syncthreads();                       // the previous draft's lanes are done with the table
            mine_build_peq(bytes + off[J.draft], m, W, Wp, L.peq, L.rowmap, L.present);
            cur_q = J.draft;
        }
        const uint32_t member = (uint32_t)(v - chunk_start[p]) * MINE_THREADS + lane;
        if (member >= J.n) continue;
        const uint32_t tj = J.r0 + member;
        const int kd = klim[J.draft], kj = klim[tj];
        const int k = (kd < 0 || kj < 0) ? -1 : max(kd, kj);
        const ConsHist H{hist_pm + hbase, hist_s + hbase, (int)J.B};
        uint32_t *row = rows + J.rows_off + (uint64_t)member * (uint32_t)(m + 1);
        const int d = chunk_lane_state<WR>(scratch, scratch_words, [&](auto &st) {
            return cons_pair<WR>(st, H, L.peq, L.rowmap, m, W, Wp, k, bytes + off[tj], len[tj], row);
        });
        dist[J.dist_off + member] = d;
    }
}

// One thread per (job, draft position p <= m): the job's members in order, rows[member][p] of those that aligned
// (dist >= 0) counted into SMX_CONS_VOTE_WORDS registers, written as the job's votes[p][...] with plain stores; thread 0
// of a job also writes aligned[job].  Neighbouring threads read neighbouring words of a row.  No atomics: the table is
// the same from run to run.  blockIdx.y strides over the jobs.
__global__ __launch_bounds__(256) void cons_vote_kernel(const int32_t *__restrict__ len, const ConsJobDev *__restrict__ jobs,
                                                        uint32_t n_jobs, const uint32_t *__restrict__ rows,
                                                        const int32_t *__restrict__ dist, uint32_t *votes,
                                                        uint32_t *aligned) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t j = blockIdx.y; j < n_jobs; j += gridDim.y) {
        const ConsJobDev J = jobs[j];
        const uint32_t words = (uint32_t)len[J.draft] + 1;
        if (p >= words) continue;
        uint32_t v[SMX_CONS_VOTE_WORDS];
#pragma unroll
        for (int x = 0; x < SMX_CONS_VOTE_WORDS; x++) v[x] = 0;
        uint32_t voters = 0;
        const uint32_t *col = rows + J.rows_off + p;
        for (uint32_t i = 0; i < J.n; i++) {
            if (dist[J.dist_off + i] < 0) continue;            // uniform over the job's threads
            voters++;
            cons_vote_word(col[(uint64_t)i * words], v);
        }
        uint32_t *out = votes + J.votes_off + (uint64_t)p * SMX_CONS_VOTE_WORDS;
#pragma unroll
        for (int x = 0; x < SMX_CONS_VOTE_WORDS; x++) out[x] = v[x];
        if (p == 0) aligned[j] = voters;
    }
}

}  // namespace smx

extern "C" int smx_launch_cons_align(void *stream, int wr, const unsigned char *d_bytes, const uint64_t *d_off,
                                     const int32_t *d_len, const int32_t *d_k, const void *d_jobs,
                                     const uint64_t *d_chunk_start, uint32_t n_jobs, int grid, uint64_t per_block,
                                     size_t lds_bytes, uint32_t *d_rows, int32_t *d_dist, void *d_hist_pm, int *d_hist_s,
                                     uint64_t hist_slice, unsigned long long *d_scratch, int scratch_words) {
    using namespace smx;
    // in the order of cons_align_kernel's parameters; every pointer is passed as the pointer it is
    void *args[] = {&d_bytes, &d_off, &d_len, &d_k, &d_jobs, &d_chunk_start, &n_jobs, &per_block, &d_rows, &d_dist,
                    &d_hist_pm, &d_hist_s, &hist_slice, &d_scratch, &scratch_words};
    auto pick = [](auto WR) { return (const void *)cons_align_kernel<WR()>; };
    return chunk_launch(stream, wr, pick, n_jobs, grid, per_block, lds_bytes, args);
}

extern "C" int smx_launch_cons_vote(void *stream, const int32_t *d_len, const void *d_jobs, uint32_t n_jobs,
                                    uint32_t max_words, const uint32_t *d_rows, const int32_t *d_dist, uint32_t *d_votes,
                                    uint32_t *d_aligned) {
    using namespace smx;
    if (n_jobs == 0 || max_words == 0) return (int)hipErrorInvalidValue;
    const dim3 grid((max_words + 255) / 256, n_jobs < 65535u ? n_jobs : 65535u);
    hipLaunchKernelGGL(cons_vote_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_len,
                       reinterpret_cast<const ConsJobDev *>(d_jobs), n_jobs, d_rows, d_dist, d_votes, d_aligned);
    return (int)hipGetLastError();
}
