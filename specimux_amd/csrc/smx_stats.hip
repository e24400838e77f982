// smx_stats.hip -- match statistics of a batch, counted on the device (specimux-stats --from-run).
//
// One thread per read (grid-stride): stats_read (smx_stats_core.h, shared with the CPU simulation) turns the read's
// lean hit records and primary record into the packed rows of the reference's stats tool.  A run has few distinct
// rows (of the order of the specimen count) and very many increments on the popular ones, so equal keys are combined
// on chip first: each workgroup counts into an LDS hash table (STATS_LCAP slots, 32-bit counts) and adds every
// occupied slot to the global table once, when it has run out of reads.  A row that finds its stretch of the LDS table
// taken goes to the global table directly.  Counts are integers: the result does not depend on arrival order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_internal.h"
#include "smx_stats_core.h"

namespace smx {

__device__ __forceinline__ void stats_global_add(uint64_t *gkeys, unsigned long long *gcounts, uint32_t gcap,
                                                 unsigned long long *dropped, uint64_t key, unsigned long long add) {
    const int s = stats_find_slot(gkeys, gcap, key, gcap < STATS_GPROBE_MAX ? gcap : STATS_GPROBE_MAX);
    if (s >= 0) atomicAdd(&gcounts[s], add);
    else atomicAdd(dropped, add);
}

__global__ __launch_bounds__(STATS_THREADS) void stats_kernel(StatsPanel P, const smx_hit *__restrict__ hits,
                                                              const smx_op *__restrict__ ops, uint32_t n_reads,
                                                              uint64_t *gkeys, unsigned long long *gcounts, uint32_t gcap,
                                                              unsigned long long *dropped, uint32_t *fallback,
                                                              uint32_t fallback_cap, uint32_t *n_fallback) {
    __shared__ uint64_t lkeys[STATS_LCAP];
    __shared__ unsigned lcnt[STATS_LCAP];
    for (int s = threadIdx.x; s < STATS_LCAP; s += STATS_THREADS) { lkeys[s] = SMX_STATS_EMPTY; lcnt[s] = 0; }
    __syncthreads();
    const size_t per_read = (size_t)2 * P.NP;
    for (uint64_t i = (uint64_t)blockIdx.x * STATS_THREADS + threadIdx.x; i < n_reads; i += (uint64_t)gridDim.x * STATS_THREADS) {
        const StatsReadInfo info = stats_read(P, hits + i * per_read, ops[i], [&](uint64_t key) {
            const int s = stats_find_slot(lkeys, STATS_LCAP, key, STATS_LPROBE);
            if (s >= 0) atomicAdd(&lcnt[s], 1u);
            else stats_global_add(gkeys, gcounts, gcap, dropped, key, 1ull);
        });
        if (info.fallback) {
            const uint32_t at = atomicAdd(n_fallback, 1u);
            if (at < fallback_cap) fallback[at] = (uint32_t)i;
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < STATS_LCAP; s += STATS_THREADS)
        if (lkeys[s] != SMX_STATS_EMPTY && lcnt[s]) stats_global_add(gkeys, gcounts, gcap, dropped, lkeys[s], lcnt[s]);
}

}  // namespace smx

extern "C" int smx_launch_stats(const smx::StatsPanel *P, void *stream, const smx_hit *d_hits, const smx_op *d_ops,
                                uint32_t n_reads, uint64_t *d_keys, uint64_t *d_counts, uint32_t cap, uint64_t *d_dropped,
                                uint32_t *d_fallback, uint32_t fallback_cap, uint32_t *d_n_fallback, int max_grid) {
    using namespace smx;
    if (n_reads == 0) return 0;
    uint64_t grid = ((uint64_t)n_reads + STATS_THREADS - 1) / STATS_THREADS;
    if (max_grid > 0 && grid > (uint64_t)max_grid) grid = (uint64_t)max_grid;
    stats_kernel<<<dim3((unsigned)grid), dim3(STATS_THREADS), 0, (hipStream_t)stream>>>(
        *P, d_hits, d_ops, n_reads, d_keys, (unsigned long long *)d_counts, cap, (unsigned long long *)d_dropped, d_fallback,
        fallback_cap, d_n_fallback);
    return (int)hipGetLastError();
}
