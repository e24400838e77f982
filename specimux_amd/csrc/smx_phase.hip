// smx_phase.hip -- the variant kernels: after cons_align_kernel and cons_vote_kernel of one smx_cons_phase call, on the
// same stream and over the rows and votes they left on the device, the sites of each job where a second allele has
// support (phase_sites_kernel), every member's allele at the kept sites as bit planes (phase_planes_kernel) and the
// co-occurrence counts of every pair of kept sites (phase_link_kernel).  DESIGN.md §18.
//
// No atomics anywhere, and every table is written in full with plain stores -- the slots past a job's kept sites as
// zeros -- so that the output is the same from run to run and needs no clearing beforehand.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_internal.h"
#include "smx_phase_core.h"

namespace smx {

constexpr unsigned PHASE_THREADS = 256;
constexpr unsigned PHASE_WAVES = PHASE_THREADS / 64;

// One workgroup per job, blockIdx.x striding over the jobs.  Thread t of round r looks at vote-table position p = r *
// PHASE_THREADS + t: its insertion site, then (p < m) its base site.  The qualifying candidates are compacted in the
// order (p, insertion before base): two wave ballots give a thread its rank inside the wave, the wave totals in LDS its
// wave's rank inside the round, and `base` carries the count over the rounds.  The first max_sites are stored.
__global__ __launch_bounds__(PHASE_THREADS) void phase_sites_kernel(const int32_t *__restrict__ len,
                                                                    const ConsJobDev *__restrict__ jobs, uint32_t n_jobs,
                                                                    const uint32_t *__restrict__ votes,
                                                                    const uint32_t *__restrict__ aligned,
                                                                    uint32_t min_permille, uint32_t min_reads,
                                                                    uint32_t max_sites, smx_cons_site *sites,
                                                                    uint32_t *n_sites, uint32_t *n_qualified) {
    __shared__ uint32_t wave_total[PHASE_WAVES];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        const ConsJobDev J = jobs[j];
        const uint32_t m = (uint32_t)len[J.draft];
        const uint32_t voters = aligned[j];
        smx_cons_site *out = sites + (uint64_t)j * max_sites;
        uint32_t base = 0;                                     // the candidates that qualified in the rounds before
        for (uint32_t p0 = 0; J.n != 0 && p0 <= m; p0 += PHASE_THREADS) {   // uniform over the workgroup
            const uint32_t p = p0 + tid;
            smx_cons_site s_ins = phase_make_site(0, 0, 0, 0, 0, 0), s_base = s_ins;
            bool q_ins = false, q_base = false;
            if (p <= m) {
                const uint32_t *v = votes + J.votes_off + (uint64_t)p * SMX_CONS_VOTE_WORDS;
                s_ins = phase_ins_site(v, p, voters);
                q_ins = phase_qualifies(s_ins.n_minor, voters, min_reads, min_permille);
                if (p < m) {
                    s_base = phase_base_site(v, p);
                    q_base = phase_qualifies(s_base.n_minor, voters, min_reads, min_permille);
                }
            }
            const uint64_t b_ins = __ballot(q_ins), b_base = __ballot(q_base);
            if (lane == 0) wave_total[wave] = (uint32_t)(__popcll(b_ins) + __popcll(b_base));
            __syncthreads();
            uint32_t at = base, total = 0;
#pragma unroll
            for (unsigned w = 0; w < PHASE_WAVES; w++) {
                const uint32_t t = wave_total[w];
                at += w < wave ? t : 0u;
                total += t;
            }
            at += (uint32_t)(__popcll(b_ins & below) + __popcll(b_base & below));
            if (q_ins) {
                if (at < max_sites) out[at] = s_ins;
                at++;
            }
            if (q_base && at < max_sites) out[at] = s_base;
            base += total;
            __syncthreads();                                   // wave_total is rewritten in the next round
        }
        const uint32_t kept = base < max_sites ? base : max_sites;
        for (uint32_t i = kept + tid; i < max_sites; i += PHASE_THREADS) out[i] = phase_make_site(0, 0, 0, 0, 0, 0);
        if (tid == 0) {
            n_sites[j] = kept;
            n_qualified[j] = base;
        }
    }
}

// One wave per (job, word of 64 members), lane = member; blockIdx.y strides over the jobs, the waves of blockIdx.x over
// the words.  Per kept site the lane reads rows[member][pos] -- unless the member is past n or above its limit, and then
// it has neither allele -- and two ballots give the words plane[site][0 = minor | 1 = major][word].  Lane 0 stores them.
__global__ __launch_bounds__(PHASE_THREADS) void phase_planes_kernel(const int32_t *__restrict__ len,
                                                                     const ConsJobDev *__restrict__ jobs, uint32_t n_jobs,
                                                                     const uint32_t *__restrict__ rows,
                                                                     const int32_t *__restrict__ dist,
                                                                     const smx_cons_site *__restrict__ sites,
                                                                     const uint32_t *__restrict__ n_sites,
                                                                     const uint64_t *__restrict__ planes_off,
                                                                     uint32_t max_sites, uint64_t *planes) {
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t word = blockIdx.x * PHASE_WAVES + (threadIdx.x >> 6);
    for (uint32_t j = blockIdx.y; j < n_jobs; j += gridDim.y) {
        const ConsJobDev J = jobs[j];
        const uint32_t words = (J.n + 63u) / 64u;
        if (word >= words) continue;                           // uniform over the wave
        const uint32_t member = word * 64u + lane;
        const bool voter = member < J.n && dist[J.dist_off + member] >= 0;
        const uint32_t *row = rows + J.rows_off + (uint64_t)member * ((uint32_t)len[J.draft] + 1u);
        const uint32_t kept = n_sites[j];
        const smx_cons_site *site = sites + (uint64_t)j * max_sites;
        uint64_t *out = planes + planes_off[j] + word;
        for (uint32_t s = 0; s < max_sites; s++) {
            uint64_t minor = 0ull, major = 0ull;
            if (s < kept) {                                    // uniform over the wave
                const smx_cons_site S = site[s];
                unsigned c = PHASE_NEITHER;
                if (voter) c = phase_classify(row[S.pos], S.kind, S.major, S.minor);
                minor = __ballot(c == PHASE_MINOR);
                major = __ballot(c == PHASE_MAJOR);
            }
            if (lane == 0) {
                out[(uint64_t)(2u * s) * words] = minor;
                out[(uint64_t)(2u * s + 1u) * words] = major;
            }
        }
    }
}

// One workgroup per job, blockIdx.x striding over the jobs; a thread per entry (s, t) of the job's max_sites x max_sites
// table: for s < t < kept the four popcounts over the job's plane words, zeros elsewhere, one 16-byte store.
__global__ __launch_bounds__(PHASE_THREADS) void phase_link_kernel(const ConsJobDev *__restrict__ jobs, uint32_t n_jobs,
                                                                   const uint32_t *__restrict__ n_sites,
                                                                   const uint64_t *__restrict__ planes_off,
                                                                   uint32_t max_sites, const uint64_t *__restrict__ planes,
                                                                   uint32_t *link) {
    for (uint32_t j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        const uint32_t words = (jobs[j].n + 63u) / 64u;
        const uint32_t kept = n_sites[j];
        const uint64_t *pl = planes + planes_off[j];
        uint4 *out = reinterpret_cast<uint4 *>(link) + (uint64_t)j * max_sites * max_sites;
        for (uint32_t e = threadIdx.x; e < max_sites * max_sites; e += PHASE_THREADS) {
            const uint32_t s = e / max_sites, t = e - s * max_sites;
            uint32_t n[4] = {0u, 0u, 0u, 0u};
            if (s < t && t < kept) {
                const uint64_t *ps = pl + (uint64_t)(2u * s) * words, *pt = pl + (uint64_t)(2u * t) * words;
                for (uint32_t w = 0; w < words; w++) phase_link_word(ps[w], ps[words + w], pt[w], pt[words + w], n);
            }
            out[e] = make_uint4(n[0], n[1], n[2], n[3]);
        }
    }
}

}  // namespace smx

extern "C" int smx_launch_cons_phase(void *stream, const int32_t *d_len, const void *d_jobs, uint32_t n_jobs,
                                     const uint32_t *d_rows, const int32_t *d_dist, const uint32_t *d_votes,
                                     const uint32_t *d_aligned, uint32_t min_permille, uint32_t min_reads,
                                     uint32_t max_sites, uint32_t max_plane_words, const uint64_t *d_planes_off,
                                     void *d_sites, uint32_t *d_n_sites, uint32_t *d_n_qualified, uint64_t *d_planes,
                                     uint32_t *d_link) {
    using namespace smx;
    if (n_jobs == 0 || max_sites == 0 || max_sites > SMX_CONS_MAX_SITES) return (int)hipErrorInvalidValue;
    const ConsJobDev *jobs = reinterpret_cast<const ConsJobDev *>(d_jobs);
    smx_cons_site *sites = reinterpret_cast<smx_cons_site *>(d_sites);
    const uint32_t per_job = n_jobs < 65535u ? n_jobs : 65535u;
    hipLaunchKernelGGL(phase_sites_kernel, dim3(per_job), dim3(PHASE_THREADS), 0, (hipStream_t)stream, d_len, jobs, n_jobs,
                       d_votes, d_aligned, min_permille, min_reads, max_sites, sites, d_n_sites, d_n_qualified);
    if (const hipError_t e = hipGetLastError()) return (int)e;
    if (max_plane_words) {                                     // no job has a member otherwise: no plane words at all
        const dim3 grid((max_plane_words + PHASE_WAVES - 1) / PHASE_WAVES, per_job);
        hipLaunchKernelGGL(phase_planes_kernel, grid, dim3(PHASE_THREADS), 0, (hipStream_t)stream, d_len, jobs, n_jobs, d_rows,
                           d_dist, (const smx_cons_site *)sites, (const uint32_t *)d_n_sites, d_planes_off, max_sites, d_planes);
        if (const hipError_t e = hipGetLastError()) return (int)e;
    }
    hipLaunchKernelGGL(phase_link_kernel, dim3(per_job), dim3(PHASE_THREADS), 0, (hipStream_t)stream, jobs, n_jobs,
                       (const uint32_t *)d_n_sites, d_planes_off, max_sites, (const uint64_t *)d_planes, d_link);
    return (int)hipGetLastError();
}
