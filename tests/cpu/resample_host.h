// The resampling kernel of specimux_amd/csrc/smx_resample.hip as a host loop, for tests/cpu/resample_sim.cpp and
// tests/asan/resample_driver.cpp: the same grid, the same indices and the same core functions (smx_resample_core.h), a
// wave being a loop over 64 lanes and its ballot a word put together bit by bit.  The buffers are the caller's, of
// exactly the sizes the plan (smx_cons_plan.h: cons_plan, cons_plan_resample) gives.
#ifndef RESAMPLE_HOST_H
#define RESAMPLE_HOST_H
#include <vector>

#include "smx_cons_plan.h"
#include "smx_resample_core.h"

namespace smx {

constexpr unsigned RESAMPLE_HOST_WAVES = 4;      // smx_resample.hip: RESAMPLE_WAVES
constexpr unsigned RESAMPLE_HOST_UNROLL = 4;     // smx_resample.hip: RESAMPLE_UNROLL

// bytes / off: the reads as the caller has them (the device has padded copies; the kernel reads the draft's bytes only)
inline void resample_host(const ConsPlan &P, const char *bytes, const uint64_t *off, uint32_t n_levels, const uint32_t *rows,
                          const int32_t *dist, const uint64_t *masks, uint64_t *agree, uint32_t *sub_aligned) {
    const uint32_t n_jobs = (uint32_t)P.jobs.size();
    const uint64_t level_stride = P.member_off.back();
    const uint32_t grid_x = n_jobs * n_levels, grid_y = (P.max_words + RESAMPLE_HOST_WAVES - 1) / RESAMPLE_HOST_WAVES;
    for (uint32_t bx = 0; bx < grid_x; bx++)
        for (uint32_t by = 0; by < grid_y; by++)
            for (uint32_t wave = 0; wave < RESAMPLE_HOST_WAVES; wave++) {
                const uint32_t j = bx / n_levels, level = bx - j * n_levels;
                const ConsJobDev &J = P.jobs[j];
                const uint32_t m = (uint32_t)P.len[J.draft], words = m + 1u;
                const uint32_t p = by * RESAMPLE_HOST_WAVES + wave;
                if (p > m) continue;
                const uint64_t *mask = masks + (uint64_t)level * level_stride + P.member_off[j];
                const uint32_t *col = rows + J.rows_off + p;
                const int32_t *d = dist + J.dist_off;
                uint64_t keeps = 0;
                for (unsigned lane = 0; lane < SMX_CONS_REPLICATES; lane++) {
                    const ResampleLane bit{lane};
                    ResampleCount c = resample_zero();
                    uint32_t packed = 0u, pending = 0u;
                    for (uint32_t i = 0; i < J.n; i++) {       // the kernel's batches of RESAMPLE_HOST_UNROLL and its flushes
                        resample_count(col[(uint64_t)i * words], d[i] >= 0 ? mask[i] : 0ull, bit, packed, c);
                        if ((i + 1) % RESAMPLE_HOST_UNROLL == 0 && i + 1 <= J.n / RESAMPLE_HOST_UNROLL * RESAMPLE_HOST_UNROLL) {
                            pending += RESAMPLE_HOST_UNROLL;
                            if (pending + RESAMPLE_HOST_UNROLL > RESAMPLE_PACK_MAX) {
                                resample_flush(packed, c);
                                pending = 0u;
                            }
                        }
                    }
                    resample_flush(packed, c);
                    const unsigned dc = p < m ? cons_code((unsigned char)bytes[off[J.draft] + p]) : 4u;
                    keeps |= (uint64_t)resample_keeps(c.a, c.del, c.ins, c.n, dc, p == m) << lane;
                    if (p == 0) sub_aligned[(uint64_t)bx * SMX_CONS_REPLICATES + lane] = c.n;
                }
                agree[P.agree_off[j] + (uint64_t)level * words + p] = keeps;
            }
}

}  // namespace smx

#endif  // RESAMPLE_HOST_H
