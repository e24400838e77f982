// smx_mine.hip -- the specimine hot path: batched HW (infix) edit distances of long reads, distance only.
//
// One chunk = one query (a full read) x up to MINE_THREADS targets (partial reads), one target per lane.
// The workgroup builds the query's Peq in LDS from a byte -> row map (row 0 = bytes absent from the query,
// all zero), then every lane runs mine_pair (smx_mine_core.h: the multi-word Myers/Hyyro bit-vector with an
// edlib-style block band, host/device code shared with the CPU unit test) over its own target.
// Matching is exact byte equality: no IUPAC equalities here (unlike the demux kernels).
//
// The per-lane state of a query of W <= WR words lives in registers (fully unrolled over WR, every index static);
// longer queries keep it in a global scratch slice per workgroup ([word][lane], coalesced).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "smx_internal.h"
#include "smx_mine_core.h"
#include "smx_mine_lds.h"   // mine_build_peq

namespace smx {

// The work is the chunk list of (job, query) pairs, pair p owning chunks [chunk_start[p], chunk_start[p + 1]) =
// MINE_THREADS targets each.  Workgroup b takes the contiguous chunks [b * per_block, (b + 1) * per_block): one pair
// search per workgroup, the Peq table rebuilt only when the query changes, and workgroups short enough that the
// hardware balances their uneven cost.  What a lane does with its distance d is the output mode:
//   DIST = false (best identity): it turns d into the pair's identity contribution (mine_identity) and, if that is
//     > 0, raises out[job.best_off + t] with a 64-bit atomic max on the bit pattern (non-negative doubles order like
//     their patterns; out starts at +0.0).
//   DIST = true (distances): it stores d at out[job.dist_off + (q - job.q0) * job.nt + t], job by job row-major.
template <bool DIST> using MineOut = std::conditional_t<DIST, int32_t, unsigned long long>;

template <int WR, bool DIST>
__global__ __launch_bounds__(MINE_THREADS) void mine_kernel(const unsigned char *__restrict__ qbytes,
                                                            const uint64_t *__restrict__ qoff,
                                                            const unsigned char *__restrict__ tbytes,
                                                            const uint64_t *__restrict__ toff,
                                                            const int32_t *__restrict__ tlen,
                                                            const MinePair *__restrict__ pairs,
                                                            const uint64_t *__restrict__ chunk_start, uint32_t n_pairs,
                                                            const MineJobDev *__restrict__ jobs,
                                                            uint64_t per_block, MineOut<DIST> *out, u64 *scratch,
                                                            int scratch_words) {
    extern __shared__ u64 lds[];
    unsigned short *rowmap = reinterpret_cast<unsigned short *>(lds);     // 512 B
    unsigned *present = reinterpret_cast<unsigned *>(lds + 64);           // 1 KiB
    u64 *peq = lds + MINE_LDS_HEAD;
    const uint64_t n_chunks = chunk_start[n_pairs];
    const uint64_t lo = (uint64_t)blockIdx.x * per_block;
    const uint64_t hi = lo + per_block < n_chunks ? lo + per_block : n_chunks;
    // the pair whose chunk range holds lo: a 64-way search, one load per lane and round (3 rounds up to 262 144
    // pairs); each wave finds the same pair on its own
    uint32_t p = 0, n = n_pairs;                   // the pair is in [p, p + n)
    while (n > 1) {
        const uint32_t step = (n + 63) / 64, idx = p + (threadIdx.x & 63) * step;
        const bool le = idx < p + n && chunk_start[idx] <= lo;    // true on a prefix of the lanes (lane 0 always)
        const uint32_t below = (uint32_t)__popcll(__ballot(le)) - 1;
        const uint32_t end = p + n;
        p += below * step;
        n = min(step, end - p);
    }
    uint32_t cur_q = 0xffffffffu;
    const unsigned lane = threadIdx.x;
    for (uint64_t v = lo; v < hi; v++) {
        while (chunk_start[p + 1] <= v) p++;
        const MinePair P = pairs[p];
        const MineJobDev J = jobs[P.job];
        const uint32_t c0 = (uint32_t)(v - chunk_start[p]) * MINE_THREADS;   // first target of the chunk in the job
        const uint64_t q0 = qoff[P.q];
        const int m = (int)(qoff[P.q + 1] - q0);
        const int W = (m + 63) >> 6, Wp = W | 1;
        if (P.q != cur_q) {
            __syncthreads();                       // the previous query's lanes are done with the table
            mine_build_peq(qbytes + q0, m, W, Wp, peq, rowmap, present);
            cur_q = P.q;
        }
        if ((uint64_t)c0 + lane < J.nt) {
            const uint32_t ti = J.t0 + c0 + lane;
            int d;
            if constexpr (WR > 0) {
                RegState<WR> st;
                d = mine_pair<WR>(st, peq, rowmap, m, W, Wp, P.k, tbytes + toff[ti], tlen[ti]);
            } else {
                u64 *sbase = scratch + (size_t)blockIdx.x * 3 * scratch_words * MINE_THREADS;
                GlobalState st{sbase + lane, sbase + (size_t)scratch_words * MINE_THREADS + lane,
                               reinterpret_cast<int *>(sbase + (size_t)2 * scratch_words * MINE_THREADS) + lane};
                d = mine_pair<0>(st, peq, rowmap, m, W, Wp, P.k, tbytes + toff[ti], tlen[ti]);
            }
            if constexpr (DIST) {
                out[J.dist_off + (uint64_t)(P.q - J.q0) * J.nt + c0 + lane] = d;
            } else {
                const double identity = mine_identity(d, m, J.min_identity);
                if (identity > 0.0) atomicMax(&out[J.best_off + c0 + lane], (unsigned long long)__double_as_longlong(identity));
            }
        }
    }
}

}  // namespace smx

extern "C" int smx_launch_mine(void *stream, int wr, int dist, const unsigned char *d_q, const uint64_t *d_qoff,
                               const unsigned char *d_t, const uint64_t *d_toff, const int32_t *d_tlen,
                               const void *d_pairs, const uint64_t *d_chunk_start, uint32_t n_pairs,
                               const void *d_jobs, int grid, uint64_t per_block, size_t lds_bytes, void *d_out,
                               unsigned long long *d_scratch, int scratch_words) {
    using namespace smx;
#define SMX_MINE_FN(WR) (dist ? (const void *)mine_kernel<WR, true> : (const void *)mine_kernel<WR, false>)
    const void *fn;
    switch (wr) {
        case 1: fn = SMX_MINE_FN(1); break;
        case 2: fn = SMX_MINE_FN(2); break;
        case 4: fn = SMX_MINE_FN(4); break;
        case 8: fn = SMX_MINE_FN(8); break;
        case 16: fn = SMX_MINE_FN(16); break;
        case 0: fn = SMX_MINE_FN(0); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef SMX_MINE_FN
    if (n_pairs == 0 || grid < 1 || per_block < 1) return (int)hipErrorInvalidValue;
    if (lds_bytes > 65536) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    // in the order of mine_kernel's parameters; every pointer is passed as the pointer it is
    void *args[] = {&d_q, &d_qoff, &d_t, &d_toff, &d_tlen, &d_pairs, &d_chunk_start, &n_pairs, &d_jobs, &per_block,
                    &d_out, &d_scratch, &scratch_words};
    return (int)hipLaunchKernel(fn, dim3(grid), dim3(MINE_THREADS), args, lds_bytes, (hipStream_t)stream);
}
