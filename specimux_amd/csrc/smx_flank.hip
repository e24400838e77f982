// smx_flank.hip -- the barcode survey's two kernels (specimux-barcodes): count what sits where the barcode should be, and
// give every distinct flank its best candidate barcode.
//
// flank_count_kernel: one lane per (read, primer, end) hit record (grid-stride): flank_of_hit (smx_flank_core.h, shared
// with the CPU simulation) cuts the flank out of the read's ASCII windows and packs it into a key.  Most of the mass sits
// on a few hundred exact barcodes and the rest is a long tail of singletons, so equal keys are combined on chip first: each
// workgroup counts into an LDS hash table (sizing: smx_flank_core.h) and adds every occupied slot to the global (key, 64-bit
// count) table once, when it has run out of hits; a key whose LDS probe run is full goes to the global table directly.
// The per-primer counters are summed in LDS and added once per workgroup.  Counts are integers: the result does not depend
// on arrival order, batch size or grid.
//
// flank_assign_kernel: one lane per key; the match words of the candidates of one primer are staged in LDS
// FLANK_ACHUNK at a time and every lane whose key belongs to that primer walks them with flank_shw.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_internal.h"
#include "smx_flank_core.h"

namespace smx {

__device__ __forceinline__ void flank_global_add(uint64_t *gkeys, unsigned long long *gcounts, uint32_t gcap,
                                                 unsigned long long *dropped, uint64_t key, unsigned long long add) {
    const int s = stats_find_slot(gkeys, gcap, key, gcap < STATS_GPROBE_MAX ? gcap : STATS_GPROBE_MAX);
    if (s >= 0) atomicAdd(&gcounts[s], add);
    else atomicAdd(dropped, add);
}

__global__ __launch_bounds__(FLANK_THREADS) void flank_count_kernel(FlankPanel P, const uint8_t *__restrict__ windows,
                                                                    int wstride, const int32_t *__restrict__ lens,
                                                                    const smx_hit *__restrict__ hits, uint32_t n_reads,
                                                                    uint64_t *gkeys, unsigned long long *gcounts, uint32_t gcap,
                                                                    unsigned long long *dropped, unsigned long long *counters) {
    __shared__ uint64_t lkeys[FLANK_LCAP];
    __shared__ unsigned lcnt[FLANK_LCAP];
    __shared__ unsigned lctr[64 * SMX_FLANK_N_COUNTERS];   // per primer; slot SMX_FLANK_HITS stays 0 until the flush
    for (int s = threadIdx.x; s < FLANK_LCAP; s += FLANK_THREADS) { lkeys[s] = SMX_STATS_EMPTY; lcnt[s] = 0; }
    for (int s = threadIdx.x; s < 64 * SMX_FLANK_N_COUNTERS; s += FLANK_THREADS) lctr[s] = 0;
    __syncthreads();
    const uint32_t H = 2u * (uint32_t)P.NP;
    const uint64_t n_items = (uint64_t)n_reads * H;
    for (uint64_t it = (uint64_t)blockIdx.x * FLANK_THREADS + threadIdx.x; it < n_items; it += (uint64_t)gridDim.x * FLANK_THREADS) {
        const uint64_t i = it / H;
        const int pe = (int)(it - i * H);
        uint64_t key;
        const int cat = flank_of_hit(P, hits[it], pe >> 1, pe & 1, lens[i], windows + i * (uint64_t)wstride, &key);
        if (cat == 0) continue;
        atomicAdd(&lctr[(pe >> 1) * SMX_FLANK_N_COUNTERS + cat], 1u);
        if (cat != SMX_FLANK_COUNTED) continue;
        const int s = stats_find_slot(lkeys, FLANK_LCAP, key, FLANK_LPROBE);
        if (s >= 0) atomicAdd(&lcnt[s], 1u);
        else flank_global_add(gkeys, gcounts, gcap, dropped, key, 1ull);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < FLANK_LCAP; s += FLANK_THREADS)
        if (lkeys[s] != SMX_STATS_EMPTY && lcnt[s]) flank_global_add(gkeys, gcounts, gcap, dropped, lkeys[s], lcnt[s]);
    for (int p = threadIdx.x; p < P.NP; p += FLANK_THREADS) {
        unsigned long long sum = 0;
        for (int c = 1; c < SMX_FLANK_N_COUNTERS; c++) {
            const unsigned v = lctr[p * SMX_FLANK_N_COUNTERS + c];
            if (v) atomicAdd(&counters[p * SMX_FLANK_N_COUNTERS + c], (unsigned long long)v);
            sum += v;
        }
        if (sum) atomicAdd(&counters[p * SMX_FLANK_N_COUNTERS + SMX_FLANK_HITS], sum);
    }
}

// cmw[c] = the four match words of candidate c, clen[c] its length, cidx[c] its index in the caller's order; the candidates
// of primer p are [pstart[p], pstart[p + 1]), in the caller's order.  Correct for keys in any order: a workgroup walks the
// lists of every primer between the least and the greatest its 256 keys hold -- one list when the keys come grouped.
__global__ __launch_bounds__(FLANK_THREADS) void flank_assign_kernel(const uint64_t *__restrict__ keys, uint32_t n_keys,
                                                                     const uint4 *__restrict__ cmw, const int *__restrict__ clen,
                                                                     const int *__restrict__ cidx, const int *__restrict__ pstart,
                                                                     int k, int32_t *__restrict__ best, int32_t *__restrict__ first,
                                                                     int32_t *__restrict__ ntied) {
    __shared__ uint4 smw[FLANK_ACHUNK];
    __shared__ int slen[FLANK_ACHUNK], sidx[FLANK_ACHUNK];
    __shared__ int prange[2];
    if (threadIdx.x == 0) { prange[0] = 64; prange[1] = -1; }
    __syncthreads();
    const uint32_t i = blockIdx.x * FLANK_THREADS + threadIdx.x;
    const bool live = i < n_keys;
    const uint64_t key = live ? keys[i] : 0;
    const int kp = live ? (int)flank_key_primer(key) : -1, flen = (int)flank_key_len(key);
    const uint64_t bits = key & ((1ull << SMX_FLANK_LEN_SHIFT) - 1);
    if (live) { atomicMin(&prange[0], kp); atomicMax(&prange[1], kp); }
    __syncthreads();
    const int p_lo = prange[0], p_hi = prange[1];
    FlankBest r = {-1, -1, 0};
    for (int p = p_lo; p <= p_hi; p++) {
        const int c0 = pstart[p], c1 = pstart[p + 1];
        for (int base = c0; base < c1; base += FLANK_ACHUNK) {
            const int n = min(FLANK_ACHUNK, c1 - base);
            __syncthreads();   // the previous chunk has been read
            for (int c = threadIdx.x; c < n; c += FLANK_THREADS) { smw[c] = cmw[base + c]; slen[c] = clen[base + c]; sidx[c] = cidx[base + c]; }
            __syncthreads();
            if (kp != p) continue;
            for (int c = 0; c < n; c++) {
                const uint4 w = smw[c];
                const uint32_t mw[4] = {w.x, w.y, w.z, w.w};
                flank_take(r, flank_shw(mw, slen[c], bits, flen), k, sidx[c]);
            }
        }
    }
    if (live) { best[i] = r.best; first[i] = r.first; ntied[i] = r.ntied; }
}

}  // namespace smx

extern "C" int smx_launch_flank_count(const smx::FlankPanel *P, void *stream, const uint8_t *d_windows, int wstride,
                                      const int32_t *d_lens, const smx_hit *d_hits, uint32_t n_reads, uint64_t *d_keys,
                                      uint64_t *d_counts, uint32_t cap, uint64_t *d_dropped, uint64_t *d_counters, int max_grid) {
    using namespace smx;
    if (n_reads == 0) return 0;
    uint64_t grid = ((uint64_t)n_reads * 2 * P->NP + FLANK_THREADS - 1) / FLANK_THREADS;
    if (max_grid > 0 && grid > (uint64_t)max_grid) grid = (uint64_t)max_grid;
    flank_count_kernel<<<dim3((unsigned)grid), dim3(FLANK_THREADS), 0, (hipStream_t)stream>>>(
        *P, d_windows, wstride, d_lens, d_hits, n_reads, d_keys, (unsigned long long *)d_counts, cap,
        (unsigned long long *)d_dropped, (unsigned long long *)d_counters);
    return (int)hipGetLastError();
}

extern "C" int smx_launch_flank_assign(void *stream, const uint64_t *d_keys, uint32_t n_keys, const void *d_cmw, const int *d_clen,
                                       const int *d_cidx, const int *d_pstart, int k, int32_t *d_best, int32_t *d_first,
                                       int32_t *d_ntied) {
    using namespace smx;
    if (n_keys == 0) return 0;
    flank_assign_kernel<<<dim3((n_keys + FLANK_THREADS - 1) / FLANK_THREADS), dim3(FLANK_THREADS), 0, (hipStream_t)stream>>>(
        d_keys, n_keys, (const uint4 *)d_cmw, d_clen, d_cidx, d_pstart, k, d_best, d_first, d_ntied);
    return (int)hipGetLastError();
}
