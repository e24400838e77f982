// smx_cons_plan.h -- the host-side plan of one smx_cons_* call (smx_calls.cpp): argument checks, the jobs with their
// offsets, the alignment's job list by register class with its chunk prefix, and the size of the history workspace.
// Host only and free of HIP calls, so that the sanitizer drivers (tests/asan/cons_driver.cpp, phase_driver.cpp,
// resample_driver.cpp, profile_driver.cpp) and the CPU simulations run it as it is.
#ifndef SMX_CONS_PLAN_H
#define SMX_CONS_PLAN_H
#include <algorithm>
#include <string>
#include <vector>

#include "smx_chunk_plan.h"
#include "smx_cons_core.h"

namespace smx {

constexpr uint64_t CONS_HIST_BYTES = (uint64_t)2 << 30;      // the history workspace of the workgroups in flight, at most
constexpr uint64_t CONS_HIST_ENTRY = sizeof(cons_pm) + sizeof(int);   // one block of one column of one lane

struct ConsPlan : ChunkLaunches {    // the launch table: the jobs of `align` per class (n), chunk_start, the grids, the scratch
    std::vector<ConsJobDev> jobs;          // the caller's jobs in the caller's order: what the vote kernel walks
    std::vector<ConsJobDev> align;         // the jobs with members, class after class (0 = generic, 1..5 = 1..16 words)
    uint64_t hist_slice = 0;               // history entries per lane of one workgroup
    uint64_t grid_cap = 1;                 // workgroups whose slices fit hist_budget
    uint64_t rows_words = 0, n_dist = 0, votes_words = 0;
    uint32_t max_words = 0;                // the longest draft's m + 1
    std::vector<int32_t> len;              // per read
    // the variant tables of an smx_cons_phase call (cons_plan_phase): job j owns the site slots [j * max_sites, (j + 1) *
    // max_sites), the 64-bit plane words [planes_off[j], planes_off[j + 1]) and the link words [j * max_sites^2 * 4, ...)
    std::vector<uint64_t> planes_off;      // n_jobs + 1 entries
    uint64_t site_slots = 0, link_words = 0;
    uint32_t max_plane_words = 0;          // the largest job's ceil(n / 64)
    // the tables of an smx_cons_resample call (cons_plan_resample): job j's members own the mask words [member_off[j],
    // member_off[j + 1]) of every level, level l starting at l * member_off[n_jobs]; its agree words are [agree_off[j],
    // agree_off[j + 1]), level after level m + 1 each; sub_aligned holds SMX_CONS_REPLICATES counts per (job, level)
    std::vector<uint64_t> member_off, agree_off;   // n_jobs + 1 entries each
    uint64_t mask_words = 0, sub_words = 0;
    // the tables of an smx_cons_profile call (cons_plan_profile)
    uint64_t member_words = 0, table_words = 0;
    uint32_t profile_max_members = 0;      // the largest job's n: the launch's second grid dimension
};

// Returns SMX_OK, or the status to fail with and why.  hist_budget: CONS_HIST_BYTES, or a test's smaller figure.
inline int cons_plan(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k, const smx_cons_job *jobs,
                     uint32_t n_jobs, uint64_t hist_budget, ConsPlan *plan, std::string *why) {
    ConsPlan &P = *plan;
    P = ConsPlan();
    P.len.assign(n_reads, 0);
    for (uint32_t r = 0; r < n_reads; r++) {
        if (roff[r + 1] < roff[r] || roff[r + 1] - roff[r] > (uint64_t)INT32_MAX) {
            *why = "read " + std::to_string(r) + ": bad offsets";
            return SMX_ERR_ARG;
        }
        P.len[r] = (int32_t)(roff[r + 1] - roff[r]);
    }
    std::vector<uint32_t> order;
    for (uint32_t j = 0; j < n_jobs; j++) {
        if (jobs[j].draft >= n_reads || (uint64_t)jobs[j].r0 + jobs[j].n > n_reads) {
            *why = "job " + std::to_string(j) + ": draft or member range out of bounds";
            return SMX_ERR_ARG;
        }
        if (P.len[jobs[j].draft] == 0) {
            *why = "job " + std::to_string(j) + ": empty draft";
            return SMX_ERR_ARG;
        }
        if (jobs[j].n) order.push_back(j);
    }
    // the member ranges may not overlap: every read has at most one row
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return jobs[a].r0 < jobs[b].r0; });
    for (size_t i = 1; i < order.size(); i++)
        if (jobs[order[i - 1]].r0 + jobs[order[i - 1]].n > jobs[order[i]].r0) {
            *why = "jobs " + std::to_string(order[i - 1]) + " and " + std::to_string(order[i]) + " overlap";
            return SMX_ERR_ARG;
        }
    P.jobs.resize(n_jobs);
    std::vector<uint32_t> by_class[6];
    for (uint32_t j = 0; j < n_jobs; j++) {
        const smx_cons_job &J = jobs[j];
        const int m = P.len[J.draft];
        // the draft's Peq table in LDS and its state class
        const ChunkTable T = chunk_table(reads + roff[J.draft], (uint64_t)m);
        if (!T.fits()) {
            *why = T.refusal("job " + std::to_string(j) + ": the draft's ");
            return SMX_ERR_UNSUPPORTED;
        }
        const int c = T.cls;
        // the history of the job's widest band over its longest banded read
        int B = 0, cols = 0;
        for (uint32_t i = 0; i < J.n; i++) {
            const uint32_t r = J.r0 + i;
            const int kp = (k[J.draft] < 0 || k[r] < 0) ? -1 : std::max(k[J.draft], k[r]);
            const int b = cons_band_blocks(m, P.len[r], kp);
            if (b > 0) { B = std::max(B, b); cols = std::max(cols, P.len[r]); }
        }
        P.jobs[j] = ConsJobDev{J.draft, J.r0, J.n, (uint32_t)B, P.rows_words, P.n_dist, P.votes_words};
        P.rows_words += (uint64_t)J.n * ((uint64_t)m + 1);
        P.n_dist += J.n;
        P.votes_words += ((uint64_t)m + 1) * SMX_CONS_VOTE_WORDS;
        P.max_words = std::max(P.max_words, (uint32_t)m + 1);
        if (J.n == 0) continue;
        P.hist_slice = std::max(P.hist_slice, (uint64_t)B * (uint64_t)cols);
        P.note(c, T.lds, T.W);
        by_class[c].push_back(j);
    }
    const uint64_t slice_bytes = P.hist_slice * MINE_THREADS * CONS_HIST_ENTRY;
    if (slice_bytes > hist_budget) {
        *why = "one workgroup's alignment history needs " + std::to_string(slice_bytes) + " bytes, more than the " +
               std::to_string(hist_budget) + " of the workspace: lower the limits k or shorten the reads";
        return SMX_ERR_UNSUPPORTED;
    }
    P.grid_cap = std::max<uint64_t>(1, hist_budget / std::max<uint64_t>(slice_bytes, 1));
    for (int c = 0; c < 6; c++) {
        // in draft order: a workgroup rebuilds the Peq table only when the draft changes
        std::stable_sort(by_class[c].begin(), by_class[c].end(), [&](uint32_t a, uint32_t b) { return jobs[a].draft < jobs[b].draft; });
        for (uint32_t j : by_class[c]) {
            P.align.push_back(P.jobs[j]);
            P.append(c, (P.jobs[j].n + MINE_THREADS - 1) / MINE_THREADS);
        }
    }
    // runs of chunks per workgroup only where the history bounds the grid: a chunk is 128 alignments with traceback,
    // and a call has few of them by the standards of the device.  Every class is capped by the history; the generic
    // class's scratch has no budget of its own here (UINT64_MAX)
    P.seal(1, UINT64_MAX, P.grid_cap);
    return SMX_OK;
}

// The variant tables of a planned call (smx_cons_phase): the argument checks and the offsets of sites, planes and link.
inline int cons_plan_phase(uint32_t min_permille, uint32_t max_sites, ConsPlan *plan, std::string *why) {
    ConsPlan &P = *plan;
    if (max_sites == 0 || max_sites > SMX_CONS_MAX_SITES) {
        *why = "max_sites " + std::to_string(max_sites) + " is not in 1.." + std::to_string(SMX_CONS_MAX_SITES);
        return SMX_ERR_ARG;
    }
    if (min_permille > 1000) {
        *why = "min_permille " + std::to_string(min_permille) + " is above 1000";
        return SMX_ERR_ARG;
    }
    P.planes_off.assign(1, 0);
    P.max_plane_words = 0;
    for (const ConsJobDev &J : P.jobs) {
        const uint32_t words = (J.n + 63) / 64;
        P.max_plane_words = std::max(P.max_plane_words, words);
        P.planes_off.push_back(P.planes_off.back() + (uint64_t)max_sites * 2 * words);
    }
    P.site_slots = (uint64_t)P.jobs.size() * max_sites;
    P.link_words = P.site_slots * max_sites * 4;
    return SMX_OK;
}

// The tables of a planned call with resampling (smx_cons_resample): the argument checks and the offsets of the members'
// mask words and of the agree words.  have_masks: the caller's mask pointer is not null.
inline int cons_plan_resample(bool have_masks, uint32_t n_levels, ConsPlan *plan, std::string *why) {
    ConsPlan &P = *plan;
    if (n_levels == 0 || n_levels > SMX_CONS_MAX_LEVELS) {
        *why = "n_levels " + std::to_string(n_levels) + " is not in 1.." + std::to_string(SMX_CONS_MAX_LEVELS);
        return SMX_ERR_ARG;
    }
    if (!have_masks && P.n_dist != 0) {
        *why = "masks is null and the jobs have " + std::to_string(P.n_dist) + " members";
        return SMX_ERR_ARG;
    }
    // the launch: a workgroup row per (job, level), four columns per workgroup
    if ((uint64_t)P.jobs.size() * n_levels > (uint64_t)INT32_MAX || P.max_words > 4u * 65535u) {
        *why = "resampling: " + std::to_string(P.jobs.size()) + " jobs x " + std::to_string(n_levels) + " levels or a draft of " +
               std::to_string(P.max_words) + " words is more than one launch holds: split the call";
        return SMX_ERR_UNSUPPORTED;
    }
    P.member_off.assign(1, 0);
    P.agree_off.assign(1, 0);
    for (const ConsJobDev &J : P.jobs) {
        P.member_off.push_back(P.member_off.back() + J.n);
        P.agree_off.push_back(P.agree_off.back() + (uint64_t)n_levels * ((uint64_t)P.len[J.draft] + 1));
    }
    P.mask_words = (uint64_t)n_levels * P.member_off.back();
    P.sub_words = (uint64_t)P.jobs.size() * n_levels * SMX_CONS_REPLICATES;
    return SMX_OK;
}

// The tables of a planned call with the error profile (smx_cons_profile): the argument checks, the sizes of the member
// words and job tables, and the launch.  Job j's members own the words [dist_off * SMX_PROFILE_MEMBER_WORDS, ...) of
// per_member, the order of member_off above, and the job the words [j * SMX_PROFILE_JOB_WORDS, ...) of tables.
// have_quals .. have_tables: the caller's pointers are not null.
inline int cons_plan_profile(bool have_quals, bool have_per_member, bool have_tables, ConsPlan *plan, std::string *why) {
    ConsPlan &P = *plan;
    if (P.n_dist != 0 && !(have_quals && have_per_member && have_tables)) {
        *why = std::string(!have_quals ? "quals" : !have_per_member ? "per_member" : "tables") + " is null and the jobs have " +
               std::to_string(P.n_dist) + " members";
        return SMX_ERR_ARG;
    }
    P.profile_max_members = 0;
    for (const ConsJobDev &J : P.jobs) P.profile_max_members = std::max(P.profile_max_members, J.n);
    // the launch: a workgroup row per job, SMX_PROFILE_BLOCK_MEMBERS members per workgroup
    if ((uint64_t)P.jobs.size() > (uint64_t)INT32_MAX || P.profile_max_members > SMX_PROFILE_BLOCK_MEMBERS * 65535u) {
        *why = "profile: " + std::to_string(P.jobs.size()) + " jobs or a job of " + std::to_string(P.profile_max_members) +
               " members is more than one launch holds: split the call";
        return SMX_ERR_UNSUPPORTED;
    }
    P.member_words = P.n_dist * SMX_PROFILE_MEMBER_WORDS;
    P.table_words = (uint64_t)P.jobs.size() * SMX_PROFILE_JOB_WORDS;
    return SMX_OK;
}

}  // namespace smx

#endif  // SMX_CONS_PLAN_H
