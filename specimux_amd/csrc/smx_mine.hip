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
#include "smx_mine_lds.h"   // the chunk walk, mine_build_peq

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
    const ChunkLds L = chunk_lds(lds);
    const ChunkSpan S = chunk_span(chunk_start, n_pairs, per_block);
    uint32_t p = chunk_owner(chunk_start, n_pairs, S.lo);      // the pair whose chunk range holds the first chunk
    uint32_t cur_q = 0xffffffffu;
    const unsigned lane = threadIdx.x;
    for (uint64_t v = S.lo; v < S.hi; v++) {
        while (chunk_start[p + 1] <= v) p++;
        const MinePair P = pairs[p];
        const MineJobDev J = jobs[P.job];
        const uint32_t c0 = (uint32_t)(v - chunk_start[p]) * MINE_THREADS;   // first target of the chunk in the job
        const uint64_t q0 = qoff[P.q];
        const int m = (int)(qoff[P.q + 1] - q0);
        const int W = (m + 63) >> 6, Wp = W | 1;
        if (P.q != cur_q) {
            __syncthreads();                       // the previous query's lanes are done with the table
            mine_build_peq(qbytes + q0, m, W, Wp, L.peq, L.rowmap, L.present);
            cur_q = P.q;
        }
        if ((uint64_t)c0 + lane < J.nt) {
            const uint32_t ti = J.t0 + c0 + lane;
            const int d = chunk_lane_state<WR>(scratch, scratch_words, [&](auto &st) {
                return mine_pair<WR>(st, L.peq, L.rowmap, m, W, Wp, P.k, tbytes + toff[ti], tlen[ti]);
            });
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
    // in the order of mine_kernel's parameters; every pointer is passed as the pointer it is
    void *args[] = {&d_q, &d_qoff, &d_t, &d_toff, &d_tlen, &d_pairs, &d_chunk_start, &n_pairs, &d_jobs, &per_block,
                    &d_out, &d_scratch, &scratch_words};
    auto pick = [&](auto WR) { return dist ? (const void *)mine_kernel<WR(), true> : (const void *)mine_kernel<WR(), false>; };
    return chunk_launch(stream, wr, pick, n_pairs, grid, per_block, lds_bytes, args);
}
