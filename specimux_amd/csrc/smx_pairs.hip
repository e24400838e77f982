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
    unsigned short *rowmap = reinterpret_cast<unsigned short *>(lds);     // 512 B
    unsigned *present = reinterpret_cast<unsigned *>(lds + 64);           // 1 KiB
    u64 *peq = lds + MINE_LDS_HEAD;
    const uint64_t n_chunks = chunk_start[n_rows];
    const uint64_t lo = (uint64_t)blockIdx.x * per_block;
    const uint64_t hi = lo + per_block < n_chunks ? lo + per_block : n_chunks;
    // the row whose chunk range holds lo: a 64-way search, one load per lane and round; each wave finds it on its own
    uint32_t p = 0, cnt = n_rows;                  // the row is in [p, p + cnt)
    while (cnt > 1) {
        const uint32_t step = (cnt + 63) / 64, idx = p + (threadIdx.x & 63) * step;
        const bool le = idx < p + cnt && chunk_start[idx] <= lo;   // true on a prefix of the lanes (lane 0 always)
        const uint32_t below = (uint32_t)__popcll(__ballot(le)) - 1;
        const uint32_t end = p + cnt;
        p += below * step;
        cnt = min(step, end - p);
    }
    uint32_t cur_q = 0xffffffffu;
    const unsigned lane = threadIdx.x;
    for (uint64_t v = lo; v < hi; v++) {
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
            mine_build_peq(bytes + off[R.read], m, W, Wp, peq, rowmap, present);
            cur_q = R.read;
        }
        const uint32_t j = c0 + lane;
        const bool active = j > i && j < J.n;
        int d = -1;
        if (active) {
            const uint32_t tj = J.r0 + j;
            const int ki = klim[R.read], kj = klim[tj];
            const int k = (ki < 0 || kj < 0) ? -1 : max(ki, kj);          // no limit on either read: none on the pair
            if constexpr (WR > 0) {
                RegState<WR> st;
                d = pairs_pair<WR>(st, peq, rowmap, m, W, Wp, k, bytes + off[tj], len[tj]);
            } else {
                u64 *sbase = scratch + (size_t)blockIdx.x * 3 * scratch_words * MINE_THREADS;
                GlobalState st{sbase + lane, sbase + (size_t)scratch_words * MINE_THREADS + lane,
                               reinterpret_cast<int *>(sbase + (size_t)2 * scratch_words * MINE_THREADS) + lane};
                d = pairs_pair<0>(st, peq, rowmap, m, W, Wp, k, bytes + off[tj], len[tj]);
            }
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
#define SMX_PAIRS_FN(WR) (dist ? (const void *)pairs_kernel<WR, true> : (const void *)pairs_kernel<WR, false>)
    const void *fn;
    switch (wr) {
        case 1: fn = SMX_PAIRS_FN(1); break;
        case 2: fn = SMX_PAIRS_FN(2); break;
        case 4: fn = SMX_PAIRS_FN(4); break;
        case 8: fn = SMX_PAIRS_FN(8); break;
        case 16: fn = SMX_PAIRS_FN(16); break;
        case 0: fn = SMX_PAIRS_FN(0); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef SMX_PAIRS_FN
    if (n_rows == 0 || grid < 1 || per_block < 1) return (int)hipErrorInvalidValue;
    if (lds_bytes > 65536) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    // in the order of pairs_kernel's parameters; every pointer is passed as the pointer it is
    void *args[] = {&d_bytes, &d_off, &d_len, &d_k, &d_rows, &d_chunk_start, &n_rows, &d_jobs, &per_block,
                    &d_out, &d_scratch, &scratch_words};
    return (int)hipLaunchKernel(fn, dim3(grid), dim3(MINE_THREADS), args, lds_bytes, (hipStream_t)stream);
}
