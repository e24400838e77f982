// smx_nearest_plan.h -- the host-side plan of one smx_nearest* call (smx_calls.cpp): argument checks, the jobs with
// their offsets, the refs by state class, the runs with their chunk prefix, the grids and the scratch size of the
// generic class.  Host only and free of HIP calls, so that the CPU simulation (tests/cpu/nearest_sim.cpp) and the
// sanitizer driver (tests/asan/nearest_driver.cpp) run it as it is.
#ifndef SMX_NEAREST_PLAN_H
#define SMX_NEAREST_PLAN_H
#include <algorithm>
#include <string>
#include <vector>

#include "smx_chunk_plan.h"
#include "smx_nearest_core.h"

namespace smx {

constexpr uint64_t NEAREST_CHUNKS_PER_CU = 32;                    // G = this x the CU count: measured, DESIGN.md §16

struct NearestPlan : ChunkLaunches {    // the launch table: the runs per class (n), chunk_start, the grids, the scratch
    std::vector<NearestJobDev> jobs;       // the caller's jobs in the caller's order
    std::vector<int32_t> len;              // per sequence
    std::vector<uint32_t> refs;            // the sequences some job takes as refs, class after class (0 = generic,
    uint32_t n_refs[6] = {0, 0, 0, 0, 0, 0};   // 1..5 = 1..16 words), in index order within a class
    std::vector<NearestRun> runs;          // class after class; first / n index the class's own ref list
    uint64_t run_len = 1;                  // the run length chosen: a (job, class) of n refs has ceil(n / run_len) runs
    uint64_t n_best = 0, n_dist = 0;       // sum(nt), sum(nq x nt)
    struct Slice { uint32_t job, lo, n; }; // a job's refs of one class: refs [lo, lo + n) of the class's list
    std::vector<Slice> slices[6];          // per class, the jobs with reads and refs of the class, in job order
};

// The first half of the plan, which needs no device: the checks, the jobs and the refs by class.  Returns SMX_OK, or the
// status to fail with and why.
inline int nearest_plan(const char *seqs, const uint64_t *off, uint32_t n_seqs, const smx_nearest_job *jobs, uint32_t n_jobs,
                        NearestPlan *plan, std::string *why) {
    NearestPlan &P = *plan;
    P = NearestPlan();
    P.len.assign(n_seqs, 0);
    for (uint32_t r = 0; r < n_seqs; r++) {
        if (off[r + 1] < off[r] || off[r + 1] - off[r] > (uint64_t)INT32_MAX) {
            *why = "sequence " + std::to_string(r) + ": bad offsets";
            return SMX_ERR_ARG;
        }
        P.len[r] = (int32_t)(off[r + 1] - off[r]);
    }
    std::vector<uint32_t> order;
    std::vector<int32_t> cover((size_t)n_seqs + 1, 0);     // +1 / -1 at the ends of every ref range
    P.jobs.resize(n_jobs);
    for (uint32_t j = 0; j < n_jobs; j++) {
        const smx_nearest_job &J = jobs[j];
        if ((uint64_t)J.q0 + J.nq > n_seqs || (uint64_t)J.t0 + J.nt > n_seqs) {
            *why = "job " + std::to_string(j) + ": ref or read range out of bounds";
            return SMX_ERR_ARG;
        }
        if (J.nt) order.push_back(j);
        if (J.nq) { cover[J.q0]++; cover[(size_t)J.q0 + J.nq]--; }
        P.jobs[j] = NearestJobDev{J.q0, J.nq, J.t0, J.nt, P.n_best, P.n_dist};
        P.n_best += J.nt;
        P.n_dist += (uint64_t)J.nq * J.nt;
    }
    // the read ranges may not overlap: every read has one entry of each output array.  Ref ranges may: many jobs over
    // one uploaded ref set
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return jobs[a].t0 < jobs[b].t0; });
    for (size_t i = 1; i < order.size(); i++)
        if ((uint64_t)jobs[order[i - 1]].t0 + jobs[order[i - 1]].nt > jobs[order[i]].t0) {
            *why = "jobs " + std::to_string(order[i - 1]) + " and " + std::to_string(order[i]) + ": read ranges overlap";
            return SMX_ERR_ARG;
        }
    // the refs by class, with the LDS their Peq tables need
    std::vector<uint32_t> by_class[6];
    int32_t depth = 0;
    for (uint32_t r = 0; r < n_seqs; r++) {
        depth += cover[r];
        if (depth <= 0) continue;
        const int m = P.len[r];
        if (m == 0) {
            *why = "sequence " + std::to_string(r) + ": an empty ref";
            return SMX_ERR_ARG;
        }
        const ChunkTable T = chunk_table(seqs + off[r], (uint64_t)m);
        if (!T.fits()) {
            *why = T.refusal("ref " + std::to_string(r) + ": ");
            return SMX_ERR_UNSUPPORTED;
        }
        const int c = T.cls;
        P.note(c, T.lds, T.W);
        by_class[c].push_back(r);
    }
    // per (job, class) the job's refs are a slice of the class list
    for (uint32_t j = 0; j < n_jobs; j++) {
        const smx_nearest_job &J = jobs[j];
        if (!J.nt || !J.nq) continue;
        for (int c = 0; c < 6; c++) {
            const auto b = by_class[c].begin(), e = by_class[c].end();
            const uint32_t lo = (uint32_t)(std::lower_bound(b, e, J.q0) - b);
            const uint32_t hi = (uint32_t)(std::lower_bound(b, e, J.q0 + J.nq) - b);   // q0 + nq <= n_seqs: no wrap
            if (hi > lo) P.slices[c].push_back(NearestPlan::Slice{j, lo, hi - lo});
        }
    }
    for (int c = 0; c < 6; c++) {
        P.n_refs[c] = (uint32_t)by_class[c].size();
        P.refs.insert(P.refs.end(), by_class[c].begin(), by_class[c].end());
    }
    return SMX_OK;
}

// The second half: the runs, their chunk prefix, the grids and the scratch size.  min_chunks: G, the chunks the call
// should have at least.  The run length is the largest that keeps sum(chunks) >= G (1 if none does), and a (job, class)
// of n refs splits them into ceil(n / run length) runs of equal length (+- 1).
inline void nearest_plan_runs(NearestPlan *plan, uint64_t min_chunks) {
    NearestPlan &P = *plan;
    P.runs.clear();                                // a plan may be given its runs more than once (the tests do)
    P.clear_records();                    // the refs nearest_plan noted stay
    uint64_t longest = 1;
    for (int c = 0; c < 6; c++)
        for (const NearestPlan::Slice &S : P.slices[c]) longest = std::max<uint64_t>(longest, S.n);
    auto chunks_at = [&](uint64_t L) {
        uint64_t total = 0;
        for (int c = 0; c < 6; c++)
            for (const NearestPlan::Slice &S : P.slices[c])
                total += ((S.n + L - 1) / L) * (((uint64_t)P.jobs[S.job].nt + MINE_THREADS - 1) / MINE_THREADS);
        return total;
    };
    // chunks_at never grows with L: the largest L in [1, longest] that still gives min_chunks, else 1
    uint64_t lo_len = 1, hi_len = longest;
    while (lo_len < hi_len) {
        const uint64_t mid = lo_len + (hi_len - lo_len + 1) / 2;
        if (chunks_at(mid) >= min_chunks) lo_len = mid; else hi_len = mid - 1;
    }
    P.run_len = lo_len;
    for (int c = 0; c < 6; c++) {
        for (const NearestPlan::Slice &S : P.slices[c]) {
            const uint64_t per_run = ((uint64_t)P.jobs[S.job].nt + MINE_THREADS - 1) / MINE_THREADS;
            const uint32_t n_runs = (uint32_t)((S.n + P.run_len - 1) / P.run_len);
            const uint32_t base = S.n / n_runs, rem = S.n % n_runs;
            uint32_t at = S.lo;
            for (uint32_t r = 0; r < n_runs; r++) {
                const uint32_t n = base + (r < rem ? 1 : 0);
                P.runs.push_back(NearestRun{S.job, at, n});
                at += n;
                P.append(c, per_run);
            }
        }
    }
    P.seal(1);                            // one chunk per workgroup; several only where the grid is capped
}

}  // namespace smx

#endif  // SMX_NEAREST_PLAN_H
