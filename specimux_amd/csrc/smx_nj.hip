// smx_nj.hip -- the neighbour-joining kernels of one smx_nj call: nj_init_kernel expands the packed
// triangle to the n x n matrix of doubles and forms the integer row sums; then, for each of the n - 3 merges, two plain
// launches on the call's stream: nj_rowmin_kernel (many workgroups, a wave per live row) leaves every row's smallest
// (Q, hi), and nj_join_kernel (one workgroup) reduces them to the pair, writes the merge record and updates the state.
//
// The arithmetic is smx_nj_core.h's, operation for operation; the selections are over the total order (Q, lo, hi), so
// the records do not depend on how the waves reduce.  The host knows the iteration count and enqueues every launch
// without waiting: no workgroup ever waits for another one, the launches' order on the stream is the only
// synchronisation between workgroups.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "smx_internal.h"
#include "smx_nj_core.h"

namespace smx {

constexpr uint32_t NJ_NONE = 0xffffffffu;   // the slot of "no candidate yet": with Q = +inf, behind every candidate

// the smallest (q, lo, hi) of the wave's first `width` lanes (a power of two), in every one of them
__device__ __forceinline__ void nj_wave_min(double &q, uint32_t &lo, uint32_t &hi, int width) {
    for (int d = width >> 1; d > 0; d >>= 1) {
        const double q2 = __shfl_xor(q, d, 64);
        const uint32_t lo2 = (uint32_t)__shfl_xor((int)lo, d, 64), hi2 = (uint32_t)__shfl_xor((int)hi, d, 64);
        if (nj_before(q2, lo2, hi2, q, lo, hi)) { q = q2; lo = lo2; hi = hi2; }
    }
}

// One workgroup per row i: d[i][*] from the triangle (the entries j < i are a column of it: strided, once per call), and
// the row's sum in 64-bit integers, converted once.
__global__ __launch_bounds__(NJ_INIT_THREADS) void nj_init_kernel(const int32_t *__restrict__ tri, uint32_t n,
                                                                  double *__restrict__ d, double *__restrict__ r,
                                                                  uint32_t *__restrict__ node) {
    __shared__ long long part[NJ_INIT_THREADS / 64];
    const uint32_t i = blockIdx.x;
    double *row = d + (size_t)i * n;
    long long sum = 0;
    for (uint32_t j = threadIdx.x; j < n; j += NJ_INIT_THREADS) {
        const int32_t v = j == i ? 0 : tri[i < j ? nj_tri_index(i, j, n) : nj_tri_index(j, i, n)];
        row[j] = (double)v;
        sum += v;
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long total = 0;
        for (unsigned w = 0; w < NJ_INIT_THREADS / 64; w++) total += part[w];
        r[i] = (double)total;
        node[i] = i;
    }
}

// A wave per live row lo <= na - 2: lane l reads d[lo][lo + 1 + l], d[lo][lo + 65 + l], ... and the r beside them
// (coalesced), keeps its smallest (Q, hi), and the wave's smallest goes to best_q[lo] / best_hi[lo].  No barrier.
__global__ __launch_bounds__(NJ_ROWMIN_THREADS) void nj_rowmin_kernel(const double *__restrict__ d,
                                                                      const double *__restrict__ r, uint32_t n, uint32_t na,
                                                                      double *__restrict__ best_q,
                                                                      uint32_t *__restrict__ best_hi) {
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t lo = blockIdx.x * NJ_ROWMIN_ROWS + (threadIdx.x >> 6);
    if (lo + 1u >= na) return;                  // uniform over the wave
    const double c = (double)(na - 2u), r_lo = r[lo];
    const double *row = d + (size_t)lo * n;
    double q = INFINITY;
    uint32_t at = lo, hi_min = NJ_NONE;
#pragma unroll 4
    for (uint32_t hi = lo + 1u + lane; hi < na; hi += 64u) {
        const double v = nj_q(c, row[hi], r_lo, r[hi]);
        if (nj_before(v, lo, hi, q, lo, hi_min)) { q = v; hi_min = hi; }
    }
    nj_wave_min(q, at, hi_min, 64);
    if (lane == 0) {
        best_q[lo] = q;
        best_hi[lo] = hi_min;
    }
}

// One workgroup; merge t, na live slots.  Thread x owns the slots k = x, x + NJ_JOIN_THREADS, ...  Four phases, a
// __syncthreads() between them; within a phase no thread reads what another writes:
//   A  the row minima 0 .. na - 2 reduced to the pair (lo, hi): reads best_*, writes LDS
//   B  every thread reads dl = d[lo][hi], ra = r[lo], rb = r[hi]; thread 0 writes the merge record.  Reads only
//   C  slot k not in {lo, hi}: reads d[lo][k], d[hi][k], r[k]; writes r[k], d[lo][k], d[k][lo] -- its own column k of the
//      rows lo and hi, and its own row k.  Thread 0 writes r[lo] and node[lo], which no thread reads in this phase
//   D  if hi is not the last slot: slot k < na - 1, k != hi: reads d[last][k] (what phase C left there); writes d[hi][k]
//      and d[k][hi].  hi != last, so the rows and columns read and written differ.  Thread 0 moves r and node
// d, r and node are written by one thread and read by another across the barriers: no __restrict__ on them.
__global__ __launch_bounds__(NJ_JOIN_THREADS) void nj_join_kernel(double *d, double *r, uint32_t *node, uint32_t n, uint32_t na,
                                                                  uint32_t t, const double *__restrict__ best_q,
                                                                  const uint32_t *__restrict__ best_hi,
                                                                  smx_nj_merge *__restrict__ merges) {
    constexpr unsigned WAVES = NJ_JOIN_THREADS / 64;
    static_assert(WAVES == 16, "the second reduction step takes 16 lanes");
    __shared__ double s_q[WAVES];
    __shared__ uint32_t s_lo[WAVES], s_hi[WAVES], s_pair[2];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // A
    double q = INFINITY;
    uint32_t lo = NJ_NONE, hi = NJ_NONE;
    for (uint32_t row = tid; row + 1u < na; row += NJ_JOIN_THREADS) {
        const double v = best_q[row];
        const uint32_t h = best_hi[row];
        if (nj_before(v, row, h, q, lo, hi)) { q = v; lo = row; hi = h; }
    }
    nj_wave_min(q, lo, hi, 64);
    if (lane == 0) { s_q[wave] = q; s_lo[wave] = lo; s_hi[wave] = hi; }
    __syncthreads();
    if (wave == 0) {
        const unsigned w = lane & (WAVES - 1u);
        q = s_q[w]; lo = s_lo[w]; hi = s_hi[w];
        nj_wave_min(q, lo, hi, (int)WAVES);
        if (lane == 0) { s_pair[0] = lo; s_pair[1] = hi; }
    }
    __syncthreads();
    lo = s_pair[0];
    hi = s_pair[1];
    if (lo >= hi || hi >= na) return;           // never with finite inputs; uniform, and nothing is indexed by a bad slot
    // B
    double *row_lo = d + (size_t)lo * n, *row_hi = d + (size_t)hi * n;
    const double dl = row_lo[hi], ra = r[lo], rb = r[hi];
    if (tid == 0) {
        smx_nj_merge m;
        m.a = node[lo]; m.b = node[hi]; m.n_active = na; m.pad = 0u;
        m.d = dl; m.ra = ra; m.rb = rb;
        merges[t] = m;
    }
    __syncthreads();
    // C
    for (uint32_t k = tid; k < na; k += NJ_JOIN_THREADS) {
        if (k == lo || k == hi) continue;
        const double a = row_lo[k], b = row_hi[k];
        const double duk = nj_duk(a, b, dl);
        r[k] = nj_r_other(r[k], a, b, duk);
        row_lo[k] = duk;
        d[(size_t)k * n + lo] = duk;
    }
    if (tid == 0) {
        r[lo] = nj_r_new(ra, rb, (double)na, dl);
        node[lo] = n + t;
    }
    __syncthreads();
    // D
    const uint32_t last = na - 1u;
    if (hi != last) {
        const double *row_last = d + (size_t)last * n;
        for (uint32_t k = tid; k < last; k += NJ_JOIN_THREADS) {
            if (k == hi) continue;
            const double v = row_last[k];
            row_hi[k] = v;
            d[(size_t)k * n + hi] = v;
        }
        if (tid == 0) {
            row_hi[hi] = 0.0;
            r[hi] = r[last];
            node[hi] = node[last];
        }
    }
}

}  // namespace smx

extern "C" int smx_launch_nj(void *stream, const int32_t *d_tri, uint32_t n, double *d_d, double *d_r, uint32_t *d_node,
                             double *d_best_q, uint32_t *d_best_hi, void *d_merges) {
    using namespace smx;
    if (n <= 3 || n > (uint32_t)SMX_NJ_MAX_N) return (int)hipErrorInvalidValue;   // nj_plan answers or refuses such a call before
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nj_init_kernel, dim3(n), dim3(NJ_INIT_THREADS), 0, s, d_tri, n, d_d, d_r, d_node);
    if (const hipError_t e = hipGetLastError()) return (int)e;
    for (uint32_t t = 0; t + 3u < n; t++) {
        const uint32_t na = n - t;
        hipLaunchKernelGGL(nj_rowmin_kernel, dim3(nj_rowmin_grid(na)), dim3(NJ_ROWMIN_THREADS), 0, s, d_d, d_r, n, na, d_best_q,
                           d_best_hi);
        hipLaunchKernelGGL(nj_join_kernel, dim3(1), dim3(NJ_JOIN_THREADS), 0, s, d_d, d_r, d_node, n, na, t, d_best_q,
                           d_best_hi, reinterpret_cast<smx_nj_merge *>(d_merges));
        if (const hipError_t e = hipGetLastError()) return (int)e;
    }
    return (int)hipSuccess;
}
