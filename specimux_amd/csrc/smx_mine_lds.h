// smx_mine_lds.h -- device code the chunked long-read kernels share (smx_mine.hip, smx_pairs.hip): the Peq table of one
// query in LDS.  Device only; the per-pair code that runs on the host too is in smx_mine_core.h / smx_pairs_core.h.
#ifndef SMX_MINE_LDS_H
#define SMX_MINE_LDS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_mine_core.h"

namespace smx {

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

}  // namespace smx

#endif  // SMX_MINE_LDS_H
