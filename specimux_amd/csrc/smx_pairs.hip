// smx_pairs.hip -- the clusters hot path: NW (global) edit distances of all pairs i < j of one specimen's reads.
//
// The layout is specimine's (smx_mine.hip): one chunk = one query (read i of a job) x up to MINE_THREADS targets (reads
// j of the same job), one target per lane; the workgroup builds the query's Peq in LDS (mine_build_peq) and every
// lane runs pairs_pair (smx_pairs_core.h) over its own target.  A job's pairs form a triangle: row i owns the chunks
// that hold a j > i, and its chunks are aligned in j -- chunk c of a job covers j in [c * MINE_THREADS,
// (c + 1) * MINE_THREADS) -- so that a wave's 64 lanes are two whole words of the row's adjacency bits.  Lanes with
// j <= i or j >= n idle.  The limit of a pair is max(k[i], k[j]), integers the host computed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_internal.h"
#include "smx_mine_lds.h"
#include "smx_pairs_core.h"

namespace smx {

// Workgroup b takes the contiguous chunks [b * per_block, (b + 1) * per_block) of the row list, row p owning chunks
// [chunk_start[p], chunk_start[p + 1]).  What a lane does with its distance d is the output mode:
//   DIST = true (distances): it stores d at out[job.out_off + i * n - i * (i + 1) / 2 + (j - i - 1)], the packed upper
//     triangle, row-major (as int32).
//   DIST = false (neighbours): the wave ballots d >= 0 and its first lane stores the two words at
//     out[job.out_off + i * ceil(n / 32) + j0 / 32 ...], plain stores of whole words: only this wave owns them.  The
//     bits of idle lanes are zero; the words left of a row's first chunk are not written (the caller zeroes the matrix
//     and mirrors the triangle).
template <int WR, bool DIST>
__global__ __launch_bounds__(MINE_THREADS) void pairs_kernel(const unsigned char *__restrict__ bytes,
                                                             const uint64_t *__restrict__ off,
                                                             const int32_t *__restrict__ len,
                                                             const int32_t *__restrict__ klim,
                                                             const PairsRow *__restrict__ rows,
                                                             const uint64_t *__restrict__ chunk_start, uint32_t n_rows,
                                                             const PairsJobDev *__restrict__ jobs, uint64_t per_block,
                                                             uint32_t *out, u64 *scratch, int scratch_words) {
    extern __shared__ u64 lds[];
    const ChunkLds L = chunk_lds(lds);
    const ChunkSpan S = chunk_span(chunk_start, n_rows, per_block);
    uint32_t p = chunk_owner(chunk_start, n_rows, S.lo);      // the row whose chunk range holds the first chunk
    uint32_t cur_q = 0xffffffffu;
    const unsigned lane = threadIdx.x;
    for (uint64_t v = S.lo; v < S.hi; v++) {
        while (chunk_start[p + 1] <= v) p++;
        const PairsRow R = rows[p];
        const PairsJobDev J = jobs[R.job];
        const uint32_t i = R.read - J.r0;                                     // the row within the job
        // the row's first chunk is the one that holds j = i + 1
        const uint32_t c0 = ((i + 1) / MINE_THREADS + (uint32_t)(v - chunk_start[p])) * MINE_THREADS;
        const int m = len[R.read];
        const int W = (m + 63) >> 6, Wp = W | 1;
        if (R.read != cur_q) {
            __syncthreads();                       // the previous query's lanes are done with the table
            mine_build_peq(bytes + off[R.read], m, W, Wp, L.peq, L.rowmap, L.present);
            cur_q = R.read;
        }
        const uint32_t j = c0 + lane;
        const bool active = j > i && j < J.n;
        int d = -1;
        if (active) {
            const uint32_t tj = J.r0 + j;
            const int ki = klim[R.read], kj = klim[tj];
            const int k = (ki < 0 || kj < 0) ? -1 : max(ki, kj);          // no limit on either read: none on the pair
            d = chunk_lane_state<WR>(scratch, scratch_words, [&](auto &st) {
                return pairs_pair<WR>(st, L.peq, L.rowmap, m, W, Wp, k, bytes + off[tj], len[tj]);
            });
        }
        if constexpr (DIST) {
            if (active) out[J.out_off + (uint64_t)i * J.n - (uint64_t)i * (i + 1) / 2 + (j - i - 1)] = (uint32_t)d;
        } else {
            const u64 bal = __ballot(active && d >= 0);
            const uint32_t nw = (J.n + 31) / 32, w0 = (c0 + (lane & 64u)) / 32;   // the wave's first word of the row
            if ((lane & 63u) == 0) {
                uint32_t *row = out + J.out_off + (uint64_t)i * nw;
                if (w0 < nw) row[w0] = (uint32_t)bal;
                if (w0 + 1 < nw) row[w0 + 1] = (uint32_t)(bal >> 32);
            }
        }
    }
}

}  // namespace smx

extern "C" int smx_launch_pairs(void *stream, int wr, int dist, const unsigned char *d_bytes, const uint64_t *d_off,
                                const int32_t *d_len, const int32_t *d_k, const void *d_rows,
                                const uint64_t *d_chunk_start, uint32_t n_rows, const void *d_jobs, int grid,
                                uint64_t per_block, size_t lds_bytes, void *d_out, unsigned long long *d_scratch,
                                int scratch_words) {
    using namespace smx;
    // in the order of pairs_kernel's parameters; every pointer is passed as the pointer it is
    void *args[] = {&d_bytes, &d_off, &d_len, &d_k, &d_rows, &d_chunk_start, &n_rows, &d_jobs, &per_block,
                    &d_out, &d_scratch, &scratch_words};
    auto pick = [&](auto WR) { return dist ? (const void *)pairs_kernel<WR(), true> : (const void *)pairs_kernel<WR(), false>; };
    return chunk_launch(stream, wr, pick, n_rows, grid, per_block, lds_bytes, args);
}
