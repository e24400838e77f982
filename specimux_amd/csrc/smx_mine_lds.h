// smx_mine_lds.h -- device code the chunked long-read kernels share (smx_mine.hip, smx_pairs.hip, smx_cons.hip,
// smx_nearest.hip, smx_hits.hip): the LDS carve, the Peq table of one query in LDS, a workgroup's walk
// over its chunks (chunk_span, chunk_owner), the per-lane state of a class (chunk_lane_state) and the launch
// (chunk_launch).  The bimera kernel (smx_reach.hip) builds no table and takes the chunk walk alone.  Device only; the per-pair code that runs on the host too is in smx_mine_core.h / smx_pairs_core.h /
// smx_cons_core.h, the host side of the calls in smx_chunk_plan.h.
#ifndef SMX_MINE_LDS_H
#define SMX_MINE_LDS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "smx_internal.h"
#include "smx_mine_core.h"

namespace smx {

// The dynamic LDS of a chunked kernel: MINE_LDS_HEAD words of head, then the Peq table.
struct ChunkLds {
    unsigned short *rowmap;   // byte -> row of the table, 0 = absent (512 B)
    unsigned *present;        // byte presence flags of the build (1 KiB)
    u64 *peq;                 // (nrows + 1) * Wp words
};

__device__ __forceinline__ ChunkLds chunk_lds(u64 *lds) {
    return ChunkLds{reinterpret_cast<unsigned short *>(lds), reinterpret_cast<unsigned *>(lds + 64), lds + MINE_LDS_HEAD};
}

// Peq of query q into LDS: rowmap[256] (byte -> row, 0 = absent), peq[(nrows + 1) * Wp] words.
__device__ void mine_build_peq(const unsigned char *qs, int m, int W, int Wp, u64 *peq, unsigned short *rowmap,
                               unsigned *present) {
    const int tid = threadIdx.x;
    for (int c = tid; c < 256; c += MINE_THREADS) present[c] = 0;
    __syncthreads();
    for (int i = tid; i < m; i += MINE_THREADS) present[qs[i]] = 1;
    __syncthreads();
    // rows 1..nrows in byte order; every wave computes the same prefix, wave 0 writes it
    const int lane = tid & 63;
    int base = 1;
    for (int c0 = 0; c0 < 256; c0 += 64) {
        const unsigned pr = present[c0 + lane];
        const u64 bal = __ballot(pr != 0);
        const int rank = __popcll(bal & ((1ull << lane) - 1ull));
        if (tid < 64) rowmap[c0 + lane] = pr ? (unsigned short)(base + rank) : (unsigned short)0;
        base += __popcll(bal);
    }
    const int words = base * Wp;                   // base = nrows + 1
    for (int i = tid; i < words; i += MINE_THREADS) peq[i] = 0ull;
    __syncthreads();
    for (int i = tid; i < m; i += MINE_THREADS) atomicOr(&peq[(size_t)rowmap[qs[i]] * Wp + (i >> 6)], 1ull << (i & 63));
    __syncthreads();
}

// The work of a launch is a list of n records, record p owning the chunks [chunk_start[p], chunk_start[p + 1]), at
// least one each.  Workgroup b takes the contiguous chunks [b * per_block, (b + 1) * per_block), short of that at the
// end of the list: one owner search per workgroup, a table rebuilt only when the pattern changes, and workgroups short
// enough that the hardware balances their uneven cost.
struct ChunkSpan { uint64_t lo, hi; };

__device__ __forceinline__ ChunkSpan chunk_span(const uint64_t *__restrict__ chunk_start, uint32_t n, uint64_t per_block) {
    const uint64_t n_chunks = chunk_start[n];
    const uint64_t lo = (uint64_t)blockIdx.x * per_block;
    return ChunkSpan{lo, lo + per_block < n_chunks ? lo + per_block : n_chunks};
}

// The record whose chunk range holds lo: the last p with chunk_start[p] <= lo.  A 64-way search, one load per lane and
// round: one round up to 64 records, two up to 4096, three up to 262 144.  Every wave finds the same record on its own.
// The ballot counts the lanes of the wave, so all 64 must be active: call it before any lane of the workgroup leaves or
// diverges, as every kernel does at its top.
__device__ __forceinline__ uint32_t chunk_owner(const uint64_t *__restrict__ chunk_start, uint32_t n, uint64_t lo) {
    uint32_t p = 0;                                // the record is in [p, p + n)
    while (n > 1) {
        const uint32_t step = chunk_owner_step(n), idx = chunk_owner_probe(p, step, threadIdx.x & 63);
        const bool le = idx < p + n && chunk_start[idx] <= lo;    // true on a prefix of the lanes (lane 0 always)
        const uint32_t count = (uint32_t)__popcll(__ballot(le));
        const uint32_t end = p + n;
        p += chunk_owner_advance(step, count);
        n = chunk_owner_left(step, end, p);
    }
    return p;
}

// The state of this lane in class WR (registers, or its columns of this workgroup's slice of scratch) handed to f(st).
template <int WR, typename F> __device__ __forceinline__ int chunk_lane_state(u64 *scratch, int scratch_words, F &&f) {
    return mine_lane_state<WR>(scratch + (size_t)blockIdx.x * 3 * scratch_words * MINE_THREADS, scratch_words, threadIdx.x, f);
}

// One launch of a chunked kernel over n records.  pick(std::integral_constant<int, WR>) names the kernel's instantiation
// for WR register words per lane (0 = state in scratch); args are the kernel's parameters in order.
template <typename Pick>
inline int chunk_launch(void *stream, int wr, Pick &&pick, uint32_t n, int grid, uint64_t per_block, size_t lds_bytes,
                        void **args) {
    const void *fn;
    switch (wr) {
        case 1: fn = pick(std::integral_constant<int, 1>()); break;
        case 2: fn = pick(std::integral_constant<int, 2>()); break;
        case 4: fn = pick(std::integral_constant<int, 4>()); break;
        case 8: fn = pick(std::integral_constant<int, 8>()); break;
        case 16: fn = pick(std::integral_constant<int, 16>()); break;
        case 0: fn = pick(std::integral_constant<int, 0>()); break;
        default: return (int)hipErrorInvalidValue;
    }
    if (n == 0 || grid < 1 || per_block < 1) return (int)hipErrorInvalidValue;
    if (lds_bytes > 65536) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    return (int)hipLaunchKernel(fn, dim3(grid), dim3(MINE_THREADS), args, lds_bytes, (hipStream_t)stream);
}

}  // namespace smx

#endif  // SMX_MINE_LDS_H
