// smx_resample.hip -- the resampling kernel: after cons_align_kernel and cons_vote_kernel of one smx_cons_resample call,
// on the same stream and over the rows and distances they left on the device, the vote of 64 subsets of each job's
// members at once, per level and column: which of the 64 replicates would call the column as the draft has it
// (smx_resample_core.h).
//
// No atomics and no LDS; every output word is written in full with plain stores, so the output is the same from run to
// run and needs no clearing beforehand.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_internal.h"
#include "smx_cons_core.h"
#include "smx_resample_core.h"

namespace smx {

constexpr unsigned RESAMPLE_THREADS = 256;
constexpr unsigned RESAMPLE_WAVES = RESAMPLE_THREADS / 64;
constexpr unsigned RESAMPLE_UNROLL = 4;
// the nibbles are flushed as soon as another batch would not fit: what is pending never exceeds RESAMPLE_PACK_MAX, and
// the fewer than RESAMPLE_UNROLL members behind the last batch fit where a batch would have
static_assert(RESAMPLE_UNROLL <= RESAMPLE_PACK_MAX, "one batch must fit a nibble");

// One wave per (job, level, column p <= m), lane = replicate: blockIdx.x = job * n_levels + level, the waves of
// blockIdx.y take RESAMPLE_WAVES neighbouring columns.  The wave walks the job's members: the distance, the row word
// rows[member][p] and the member's mask word of the level are the same for all lanes (scalar loads), the lane counts the
// word under its own bit of the mask.  A member above its limit counts for no replicate.  After the walk one ballot of
// resample_keeps is the (job, level, column)'s agree word, stored by lane 0; the wave of column 0 also stores every
// lane's voters to sub_aligned[job][level][lane].  A job without members: all-ones words, zero counts.
__global__ __launch_bounds__(RESAMPLE_THREADS) void cons_resample_kernel(const unsigned char *__restrict__ bytes,
                                                                         const uint64_t *__restrict__ off,
                                                                         const int32_t *__restrict__ len,
                                                                         const ConsJobDev *__restrict__ jobs,
                                                                         uint32_t n_levels,
                                                                         const uint32_t *__restrict__ rows,
                                                                         const int32_t *__restrict__ dist,
                                                                         const uint64_t *__restrict__ masks,
                                                                         const uint64_t *__restrict__ member_off,
                                                                         const uint64_t *__restrict__ agree_off,
                                                                         uint64_t level_stride, uint64_t *agree,
                                                                         uint32_t *sub_aligned) {
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t j = blockIdx.x / n_levels, level = blockIdx.x - j * n_levels;
    const ConsJobDev J = jobs[j];
    const uint32_t m = (uint32_t)len[J.draft], words = m + 1u;
    const uint32_t p = blockIdx.y * RESAMPLE_WAVES + wave;
    if (p > m) return;                                         // uniform over the wave
    const uint64_t *mask = masks + (uint64_t)level * level_stride + member_off[j];
    const uint32_t *col = rows + J.rows_off + p;            // the column's word of member 0; a row further per member
    const int32_t *d = dist + J.dist_off;
    // a wave-uniform 64-bit word is a lane mask as it stands: lane b reads bit b of it
    const auto bit = [](uint64_t word) -> uint32_t { return (uint32_t)__builtin_amdgcn_inverse_ballot_w64(word); };
    ResampleCount c = resample_zero();
    uint32_t packed = 0u, pending = 0u;                        // members counted into the nibbles since the last flush
    // A member above its limit is skipped by a mask word of zero, not by a branch (the test is uniform either way): the
    // loads of RESAMPLE_UNROLL members are then in flight together.  Such a member's row is stale workspace, read and
    // counted for nobody.
    const uint64_t stride = words;
    uint32_t i = 0;
    for (; i + RESAMPLE_UNROLL <= J.n; i += RESAMPLE_UNROLL) {
        int32_t di[RESAMPLE_UNROLL];
        uint64_t mi[RESAMPLE_UNROLL];
        uint32_t wi[RESAMPLE_UNROLL];
#pragma unroll
        for (unsigned u = 0; u < RESAMPLE_UNROLL; u++) {
            di[u] = d[i + u];
            mi[u] = mask[i + u];
            wi[u] = col[u * stride];
        }
        col += RESAMPLE_UNROLL * stride;
#pragma unroll
        for (unsigned u = 0; u < RESAMPLE_UNROLL; u++) resample_count(wi[u], di[u] >= 0 ? mi[u] : 0ull, bit, packed, c);
        pending += RESAMPLE_UNROLL;
        if (pending + RESAMPLE_UNROLL > RESAMPLE_PACK_MAX) {   // uniform over the wave
            resample_flush(packed, c);
            pending = 0u;
        }
    }
    for (; i < J.n; i++, col += stride) {                      // fewer than RESAMPLE_UNROLL: they fit the nibbles
        const uint64_t mw = mask[i];
        resample_count(col[0], d[i] >= 0 ? mw : 0ull, bit, packed, c);
    }
    resample_flush(packed, c);
    const unsigned dc = p < m ? cons_code(bytes[off[J.draft] + p]) : 4u;
    const uint64_t keeps = __ballot(resample_keeps(c.a, c.del, c.ins, c.n, dc, p == m));
    if (lane == 0) agree[agree_off[j] + (uint64_t)level * words + p] = keeps;
    if (p == 0) sub_aligned[(uint64_t)blockIdx.x * SMX_CONS_REPLICATES + lane] = c.n;
}

}  // namespace smx

extern "C" int smx_launch_cons_resample(void *stream, const unsigned char *d_bytes, const uint64_t *d_off,
                                        const int32_t *d_len, const void *d_jobs, uint32_t n_jobs, uint32_t n_levels,
                                        uint32_t max_words, const uint32_t *d_rows, const int32_t *d_dist,
                                        const uint64_t *d_masks, const uint64_t *d_member_off, const uint64_t *d_agree_off,
                                        uint64_t level_stride, uint64_t *d_agree, uint32_t *d_sub_aligned) {
    using namespace smx;
    const uint64_t gx = (uint64_t)n_jobs * n_levels, gy = ((uint64_t)max_words + RESAMPLE_WAVES - 1) / RESAMPLE_WAVES;
    if (gx == 0 || gx > 0x7fffffffull || gy == 0 || gy > 65535ull || n_levels > SMX_CONS_MAX_LEVELS)
        return (int)hipErrorInvalidValue;                      // cons_plan_resample refuses such a call before
    hipLaunchKernelGGL(cons_resample_kernel, dim3((uint32_t)gx, (uint32_t)gy), dim3(RESAMPLE_THREADS), 0, (hipStream_t)stream,
                       d_bytes, d_off, d_len, reinterpret_cast<const ConsJobDev *>(d_jobs), n_levels, d_rows, d_dist, d_masks,
                       d_member_off, d_agree_off, level_stride, d_agree, d_sub_aligned);
    return (int)hipGetLastError();
}
