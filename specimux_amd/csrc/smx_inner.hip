// smx_inner.hip -- the inner scan (smx_inner_scan): every pattern against the whole read, hits on the internal columns.
//
// inner_scan_kernel: one lane = one (read, piece) unit x the G patterns of one pass (blockIdx.y).  The units of all reads
// of a chunk are flattened over the lanes by a prefix sum over the reads' piece counts (unit_read / ustart, built by
// the host), so a 650-nt read fills four or five lanes and a 20 000-nt read a few hundred.  The workgroup keeps the
// byte -> code map and the pass's match words (16 codes x G) in LDS; a lane keeps Pv, Mv, the last-row value and the run
// tracker of its G patterns in registers and reads its bases 16 bytes at a time (smx_inner_core.h, inner_scan_piece).
// inner_merge_kernel: one lane per (read, pattern) joins the records of the read's units (inner_merge).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_internal.h"
#include "smx_inner_core.h"

namespace smx {

template <typename W, int G>
__global__ __launch_bounds__(INNER_THREADS) void inner_scan_kernel(InnerArgs A) {
    __shared__ W s_peq[16 * G];
    __shared__ unsigned char s_lut[256];
    __shared__ int s_m[G], s_k[G], s_j[G];
    const int tid = threadIdx.x;
    const size_t pass = blockIdx.y;
    s_lut[tid] = A.lut[tid];
    if (tid < 16 * G) s_peq[tid] = reinterpret_cast<const W *>(A.peq)[pass * 16 * G + tid];
    if (tid < G) {
        s_m[tid] = A.pm[pass * G + tid];
        s_k[tid] = A.pk[pass * G + tid];
        s_j[tid] = A.jmap[pass * G + tid];
    }
    __syncthreads();
    const uint64_t unit = (uint64_t)blockIdx.x * INNER_THREADS + tid;
    if (unit >= A.n_units) return;
    const uint32_t r = A.unit_read[unit];
    const int piece = (int)((uint32_t)unit - A.ustart[r]);
    const uint64_t roff = A.roff[r];
    const int n = (int)(A.roff[r + 1] - roff);
    inner_scan_piece<W, G>(s_peq, s_lut, s_m, s_k, s_j, A.bases, roff, n, A.margin, A.PL, A.lead, piece, A.H,
                           A.recs + unit * (uint64_t)A.Q * (uint64_t)inner_rec_words(A.H));
}

__global__ __launch_bounds__(INNER_THREADS) void inner_merge_kernel(InnerArgs A, uint32_t n_reads, uint8_t *nhit,
                                                                    int8_t *hit_dist, int32_t *hit_end) {
    const uint64_t t = (uint64_t)blockIdx.x * INNER_THREADS + threadIdx.x;
    if (t >= (uint64_t)n_reads * (uint64_t)A.Q) return;
    const uint32_t r = (uint32_t)(t / (uint64_t)A.Q);
    const int j = (int)(t - (uint64_t)r * (uint64_t)A.Q);
    const uint32_t u0 = A.ustart[r];
    inner_merge(A.recs, u0, (int)(A.ustart[r + 1] - u0), A.Q, j, A.H, A.margin, A.PL, nhit + t, hit_dist + t * A.H,
                hit_end + t * A.H);
}

}  // namespace smx

extern "C" int smx_launch_inner_scan(void *stream, int w64, int G, int npass, const smx::InnerArgs *A) {
    using namespace smx;
    const void *fn;
    if (G == 4) fn = w64 ? (const void *)inner_scan_kernel<uint64_t, 4> : (const void *)inner_scan_kernel<uint32_t, 4>;
    else if (G == 8) fn = w64 ? (const void *)inner_scan_kernel<uint64_t, 8> : (const void *)inner_scan_kernel<uint32_t, 8>;
    else return (int)hipErrorInvalidValue;
    if (A->n_units == 0 || npass < 1 || npass > 65535) return (int)hipErrorInvalidValue;
    const uint64_t grid = ((uint64_t)A->n_units + INNER_THREADS - 1) / INNER_THREADS;
    InnerArgs a = *A;
    void *args[] = {&a};
    return (int)hipLaunchKernel(fn, dim3((unsigned)grid, (unsigned)npass), dim3(INNER_THREADS), args, 0, (hipStream_t)stream);
}

extern "C" int smx_launch_inner_merge(void *stream, const smx::InnerArgs *A, uint32_t n_reads, uint8_t *d_nhit,
                                      int8_t *d_hit_dist, int32_t *d_hit_end) {
    using namespace smx;
    const uint64_t n = (uint64_t)n_reads * (uint64_t)A->Q;
    if (n == 0) return (int)hipErrorInvalidValue;
    const uint64_t grid = (n + INNER_THREADS - 1) / INNER_THREADS;
    if (grid > 0x7fffffffull) return (int)hipErrorInvalidValue;
    InnerArgs a = *A;
    void *args[] = {&a, &n_reads, &d_nhit, &d_hit_dist, &d_hit_end};
    return (int)hipLaunchKernel((const void *)inner_merge_kernel, dim3((unsigned)grid), dim3(INNER_THREADS), args, 0,
                                (hipStream_t)stream);
}
