// smx_profile.hip -- the error-profile kernel: after cons_align_kernel and cons_vote_kernel of one smx_cons_profile call,
// on the same stream and over the rows and distances they left on the device, every member's row read once against its
// job's draft and the read's quality bytes: the member's eight counts and the job's q / subst / ins / hp tables
// (smx_profile_core.h).
//
// Integer adds only: the member words are plain stores, the job tables are summed in LDS (ds_add) and added to the
// zeroed global tables with one atomic per nonzero word and workgroup, so every output word is the same from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_internal.h"
#include "smx_cons_core.h"
#include "smx_profile_core.h"

namespace smx {

constexpr unsigned PROFILE_THREADS = 256;
constexpr unsigned PROFILE_WAVES = PROFILE_THREADS / 64;
static_assert(PROFILE_WAVES * SMX_PROFILE_WAVE_MEMBERS == SMX_PROFILE_BLOCK_MEMBERS, "the plan's members per workgroup");

// inclusive scans over the wave's 64 lanes
__device__ __forceinline__ uint32_t profile_scan_add(uint32_t v, unsigned lane) {
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ uint32_t profile_scan_max(uint32_t v, unsigned lane) {
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= d && t > v) v = t;
    }
    return v;
}

// One workgroup per (job, SMX_PROFILE_BLOCK_MEMBERS of its members): blockIdx.x = job, blockIdx.y = the slice; wave w takes
// the slice's members w, w + PROFILE_WAVES, ...  A wave walks its member's row in batches of 64 columns, lane = column,
// so the row-major row is read coalesced, once (the word behind each column, which the run's last column needs, is a second
// load of the same lines).  Three values are carried from batch to batch, each the last lane's: the read bytes consumed so
// far (a scan of c_p), the first column of the stretch of equal draft codes that is open (a max scan of the stretch
// starts) and that stretch's observed length so far.  c_p <= 256 and a column's share of its run <= 9, so one scan of
// c | share << 16 serves both.  The draft's runs are found here, from three neighbouring draft bytes per lane: a host table
// of them would be one more upload per call, for what a scan the wave makes anyway gives.
//
// Tables: `tab` is the workgroup's copy of the job's SMX_PROFILE_JOB_WORDS; the q counts of the member in hand go to the
// wave's own `wq` first and reach `tab` only when the row held no clipped length.  The match diagonal of subst, four
// entries that nearly every column would add to, is counted per lane in two registers of 16-bit fields instead and added
// once per member (a lane sees one column per batch: 65 535 batches, drafts of four million bases, before a field is full;
// cons_plan admits no draft whose Peq table does not fit the LDS, far below that).
__global__ __launch_bounds__(PROFILE_THREADS) void cons_profile_kernel(const unsigned char *__restrict__ bytes,
                                                                       const uint64_t *__restrict__ off,
                                                                       const int32_t *__restrict__ len,
                                                                       const ConsJobDev *__restrict__ jobs,
                                                                       const uint32_t *__restrict__ rows,
                                                                       const int32_t *__restrict__ dist,
                                                                       const unsigned char *__restrict__ quals,
                                                                       const uint64_t *__restrict__ qoff,
                                                                       uint32_t *__restrict__ per_member,
                                                                       uint32_t *__restrict__ tables) {
    __shared__ uint32_t tab[SMX_PROFILE_JOB_WORDS];
    __shared__ uint32_t wq_all[PROFILE_WAVES][PROFILE_Q_WORDS];
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t j = blockIdx.x;
    const ConsJobDev J = jobs[j];
    const uint32_t first = blockIdx.y * SMX_PROFILE_BLOCK_MEMBERS;
    if (first >= J.n) return;                                  // uniform over the workgroup, before any barrier
    for (unsigned x = threadIdx.x; x < SMX_PROFILE_JOB_WORDS; x += PROFILE_THREADS) tab[x] = 0u;
    uint32_t *wq = wq_all[wave];
    for (unsigned x = lane; x < PROFILE_Q_WORDS; x += 64) wq[x] = 0u;
    __syncthreads();
    const uint32_t m = (uint32_t)len[J.draft];
    const unsigned char *draft = bytes + off[J.draft];
    const auto add_tab = [&](unsigned at, uint32_t v) { atomicAdd(&tab[at], v); };
    const auto add_wq = [&](unsigned at, uint32_t v) { atomicAdd(&wq[at - PROFILE_Q], v); };
    for (uint32_t i = first + wave; i < J.n && i < first + SMX_PROFILE_BLOCK_MEMBERS; i += PROFILE_WAVES) {   // uniform over the wave
        uint32_t *out = per_member + (J.dist_off + i) * (uint64_t)SMX_PROFILE_MEMBER_WORDS;
        if (dist[J.dist_off + i] < 0) {                        // above its limit: no row, eight zeros
            if (lane < SMX_PROFILE_MEMBER_WORDS) out[lane] = 0u;
            continue;
        }
        const uint32_t r = J.r0 + i;
        const uint32_t *row = rows + J.rows_off + (uint64_t)i * ((uint64_t)m + 1u);
        const unsigned char *qual = quals + qoff[r];
        const uint32_t rlen = (uint32_t)(qoff[r + 1] - qoff[r]);
        uint32_t n_sub = 0u, n_del = 0u, n_other = 0u, n_events = 0u, clipped = 0u;
        uint32_t diag_ac = 0u, diag_gt = 0u;   // this lane's match columns by draft code, 16 bits each: a lane has one column per batch
        uint32_t consumed = 0u, open_start1 = 0u, open_sum = 0u;    // the three carries; starts are kept as column + 1
        for (uint32_t b0 = 0; b0 <= m; b0 += 64) {
            const uint32_t p = b0 + lane;
            const uint32_t w = p <= m ? row[p] : 0u;
            const uint32_t wn = p < m ? row[p + 1] : 0u;
            const unsigned dc = p < m ? cons_code(draft[p]) : PROFILE_NO_CODE;
            const unsigned dprev = p > 0 && p <= m ? cons_code(draft[p - 1]) : PROFILE_NO_CODE;
            const unsigned dnext = p + 1 < m ? cons_code(draft[p + 1]) : PROFILE_NO_CODE;
            const unsigned cls = profile_class(w, dc, p, m);
            const unsigned L = p <= m ? profile_len(w) : 0u;
            n_sub += (uint32_t)__popcll(__ballot(cls == PROFILE_SUB));
            n_del += (uint32_t)__popcll(__ballot(cls == PROFILE_DEL));
            n_other += (uint32_t)__popcll(__ballot(cls == PROFILE_OTHER));
            n_events += (uint32_t)__popcll(__ballot(L != 0u));
            clipped |= __ballot(L == 255u) != 0ull ? 1u : 0u;
            // subst and ins: no read position needed
            if (cls == PROFILE_MATCH) {
                const uint32_t one = 1u << ((dc & 1u) << 4);
                diag_ac += dc < 2u ? one : 0u;
                diag_gt += dc < 2u ? 0u : one;
            } else {
                const int at = profile_subst_index(w, dc, p, m);
                if (at >= 0) add_tab((unsigned)at, 1u);
            }
            if (L != 0u) profile_ins(w, add_tab);
            // the read position and the runs
            const bool starts = profile_starts(dprev, dc, p, m), ends = profile_ends_run(dc, dnext, p, m);
            const uint32_t c = profile_consumed(w, p, m), share = profile_run_votes(w, wn, dc, ends, p, m);
            const uint32_t incl = profile_scan_add(c | (share << 16), lane);
            const uint32_t c_incl = incl & 0xffffu, s_incl = incl >> 16;
            const uint32_t rp = consumed + (c_incl - c) + L;
            if (!clipped) profile_q(w, cls, rp, qual, rlen, add_wq);   // a clipped length further on: wq is dropped below
            const uint32_t scan1 = profile_scan_max(starts ? p + 1u : 0u, lane);
            const uint32_t start1 = scan1 > open_start1 ? scan1 : open_start1;    // 0 only where p >= m follows no column
            const uint32_t start = start1 - 1u;
            const unsigned from = start1 != 0u && start >= b0 ? start - b0 : 0u;
            const uint32_t excl_at_start = (uint32_t)__shfl((int)(s_incl - share), (int)from, 64);
            const uint32_t sum = profile_stretch_sum(s_incl, excl_at_start, open_sum, start, b0);
            if (ends) add_tab(profile_hp_index(p + 1u - start, sum), 1u);
            consumed += (uint32_t)__shfl((int)c_incl, 63, 64);
            open_start1 = (uint32_t)__shfl((int)start1, 63, 64);
            open_sum = (uint32_t)__shfl((int)sum, 63, 64);
        }
        // the match diagonal of subst: at most four adds per lane and member, where the columns would have made one each
        if (diag_ac & 0xffffu) add_tab(PROFILE_SUBST + 0u, diag_ac & 0xffffu);
        if (diag_ac >> 16) add_tab(PROFILE_SUBST + 6u, diag_ac >> 16);
        if (diag_gt & 0xffffu) add_tab(PROFILE_SUBST + 12u, diag_gt & 0xffffu);
        if (diag_gt >> 16) add_tab(PROFILE_SUBST + 18u, diag_gt >> 16);
        if (lane == 0) {
            const uint32_t n_match = m - (n_sub + n_del + n_other);                // every column has one class
            const uint32_t n_bases = consumed - (n_match + n_sub + n_other);      // sum of L_p as stored
            const uint4 lo = make_uint4(n_match, n_sub, n_del, n_other), hi = make_uint4(n_events, n_bases, clipped, 0u);
            reinterpret_cast<uint4 *>(out)[0] = lo;
            reinterpret_cast<uint4 *>(out)[1] = hi;
        }
        // the member's q counts: kept unless it is clipped; zero again for the next member either way.  Each lane reads
        // and clears the words it alone adds here, after the wave's own ds_adds to them
        __builtin_amdgcn_wave_barrier();
        for (unsigned x = lane; x < PROFILE_Q_WORDS; x += 64) {
            const uint32_t v = wq[x];
            if (v != 0u) {
                if (!clipped) atomicAdd(&tab[PROFILE_Q + x], v);
                wq[x] = 0u;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    uint32_t *job_tab = tables + (uint64_t)j * SMX_PROFILE_JOB_WORDS;
    for (unsigned x = threadIdx.x; x < SMX_PROFILE_JOB_WORDS; x += PROFILE_THREADS)
        if (tab[x]) atomicAdd(&job_tab[x], tab[x]);
}

}  // namespace smx

extern "C" int smx_launch_cons_profile(void *stream, const unsigned char *d_bytes, const uint64_t *d_off, const int32_t *d_len,
                                       const void *d_jobs, uint32_t n_jobs, uint32_t max_members, const uint32_t *d_rows,
                                       const int32_t *d_dist, const unsigned char *d_quals, const uint64_t *d_qoff,
                                       uint32_t *d_per_member, uint32_t *d_tables) {
    using namespace smx;
    const uint64_t gy = ((uint64_t)max_members + SMX_PROFILE_BLOCK_MEMBERS - 1) / SMX_PROFILE_BLOCK_MEMBERS;
    if (n_jobs == 0 || n_jobs > 0x7fffffffu || gy > 65535ull) return (int)hipErrorInvalidValue;   // cons_plan_profile refuses such a call before
    if (gy == 0) return (int)hipSuccess;                       // no job has members: the zeroed tables are the result
    hipLaunchKernelGGL(cons_profile_kernel, dim3(n_jobs, (uint32_t)gy), dim3(PROFILE_THREADS), 0, (hipStream_t)stream, d_bytes,
                       d_off, d_len, reinterpret_cast<const ConsJobDev *>(d_jobs), d_rows, d_dist, d_quals, d_qoff, d_per_member,
                       d_tables);
    return (int)hipGetLastError();
}
