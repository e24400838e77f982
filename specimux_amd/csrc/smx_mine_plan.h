// smx_mine_plan.h -- the host-side plan of one smx_mine_* call (smx_calls.cpp): argument checks, the padded targets, the
// jobs with their output offsets, the (job, query) records by state class with their chunk prefix, the grids and the
// scratch size of the generic class.  Host only and free of HIP calls, so that the CPU simulation
// (tests/cpu/mine_plan_sim.cpp) and the sanitizer driver (tests/asan/mine_driver.cpp) run it as it is.
#ifndef SMX_MINE_PLAN_H
#define SMX_MINE_PLAN_H
#include <algorithm>
#include <string>
#include <vector>

#include "smx_chunk_plan.h"

namespace smx {

// A workgroup takes MINE_BLOCK_CHUNKS chunks in a row (more where the grid is capped): the pair search and the Peq
// build of a query's run of chunks are paid once.  Measured on MI355X: one chunk per workgroup loses
// 1.5x on runs of cheap (decoy) chunks, runs of 8 lose ~11 % to balance on costly chunks
constexpr uint64_t MINE_BLOCK_CHUNKS = 8;

struct MinePlan : ChunkLaunches {    // the launch table: the pairs per class (n), chunk_start, the grids, the scratch
    std::vector<uint64_t> tdoff;           // the targets as the kernel reads them (chunk_padded_sequences)
    std::vector<int32_t> tlen;
    std::vector<unsigned char> tpad;
    std::vector<MineJobDev> jobs;          // the caller's jobs in the caller's order, with their output offsets
    std::vector<MinePair> pairs;           // class after class (0 = generic, 1..5 = 1..16 words), by query within a class
    uint64_t n_dist = 0, n_best = 0;       // sum(nq x nt), sum(nt): the output elements of the two modes
};

// The plan of a call.  scratch_budget: the bytes the generic class's state may take (CHUNK_SCRATCH_BYTES in
// production).  Returns SMX_OK, or the status to fail with and why.
inline int mine_plan(const char *queries, const uint64_t *qoff, uint32_t n_queries, const int32_t *k, const char *targets,
                     const uint64_t *toff, uint32_t n_targets, const smx_mine_job *jobs, uint32_t n_jobs,
                     uint64_t scratch_budget, MinePlan *plan, std::string *why) {
    MinePlan &P = *plan;
    P = MinePlan();
    std::vector<size_t> qlds;
    std::vector<int> qclass;
    int rc = chunk_pattern_classes(queries, qoff, n_queries, false, &qlds, &qclass, why);
    if (rc != SMX_OK) return rc;
    rc = chunk_padded_sequences(targets, toff, n_targets, &P.tdoff, &P.tlen, &P.tpad, why);
    if (rc != SMX_OK) return rc;
    // jobs -> (job, query) pairs with at least one target, grouped by register class, in query order within a class
    // (a workgroup rebuilds the Peq table only when the query changes)
    P.jobs.resize(n_jobs);
    std::vector<MinePair> pairs[6];
    for (uint32_t j = 0; j < n_jobs; j++) {
        const smx_mine_job &J = jobs[j];
        if ((uint64_t)J.q0 + J.nq > n_queries || (uint64_t)J.t0 + J.nt > n_targets) {
            *why = "job " + std::to_string(j) + ": query or target range out of bounds";
            return SMX_ERR_ARG;
        }
        P.jobs[j] = MineJobDev{J.q0, J.nq, J.t0, J.nt, P.n_dist, P.n_best, J.min_identity};
        P.n_dist += (uint64_t)J.nq * J.nt;
        P.n_best += J.nt;
        if (J.nt == 0) continue;
        for (uint32_t i = 0; i < J.nq; i++) {
            const uint32_t q = J.q0 + i;
            const int c = qclass[q];
            P.note(c, qlds[q], (size_t)((qoff[q + 1] - qoff[q] + 63) / 64));
            pairs[c].push_back(MinePair{j, q, k[q], 0});
        }
    }
    for (int c = 0; c < 6; c++) {
        std::stable_sort(pairs[c].begin(), pairs[c].end(), [](const MinePair &a, const MinePair &b) { return a.q < b.q; });
        for (const MinePair &R : pairs[c]) P.append(c, ((uint64_t)P.jobs[R.job].nt + MINE_THREADS - 1) / MINE_THREADS);
        P.pairs.insert(P.pairs.end(), pairs[c].begin(), pairs[c].end());
    }
    // MINE_BLOCK_CHUNKS chunks per workgroup; more only where the grid is capped: by the launch, and in the generic class by
    // the scratch slices of the workgroups in flight
    P.seal(MINE_BLOCK_CHUNKS, scratch_budget);
    return SMX_OK;
}

}  // namespace smx

#endif  // SMX_MINE_PLAN_H
