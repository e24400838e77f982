// smx_reach_plan.h -- the host-side plan of one smx_prefix_reach* call (smx_calls.cpp): argument checks, the jobs with
// their output offsets, one work record per (job, query) with the chunk prefix, the grid, and the sequences as the
// kernel reads them.  Host only and free of HIP calls, so that the CPU simulation
// (tests/cpu/reach_sim.cpp) and the sanitizer driver (tests/asan/reach_driver.cpp) run it as it is.
#ifndef SMX_REACH_PLAN_H
#define SMX_REACH_PLAN_H
#include <algorithm>
#include <string>
#include <vector>

#include "smx_chunk_plan.h"
#include "smx_reach_core.h"

namespace smx {

constexpr uint64_t REACH_BLOCK_CHUNKS = 4;         // chunks a workgroup takes in a row: one record search for 512 (pair, side) items

struct ReachPlan {
    std::vector<ReachJobDev> jobs;         // the caller's jobs in the caller's order
    std::vector<int32_t> len;              // per sequence
    std::vector<ReachRec> recs;            // job after job, query after query: the queries of jobs with targets
    std::vector<uint64_t> chunk_start;     // the records' chunk prefix, n + 1 entries (empty without records)
    uint64_t chunks = 0, grid = 0, per_block = 1;
    uint64_t n_rows = 0, n_pairs = 0;      // sum(nq), sum(nq x nt)
    uint64_t n_keys = 0, n_values = 0;     // n_rows x 2 x (E + 1) x REACH_SLOTS keys; n_pairs x 2 x (E + 1) values (matrix mode)
};

// The plan of a call, from the offsets alone.  Returns SMX_OK, or the status to fail with and why.
inline int reach_plan(const uint64_t *off, uint32_t n_seqs, const smx_reach_job *jobs, uint32_t n_jobs, uint32_t E,
                      ReachPlan *plan, std::string *why) {
    ReachPlan &P = *plan;
    P = ReachPlan();
    if (E > (uint32_t)REACH_MAX_E) {
        *why = "E = " + std::to_string(E) + " outside 0.." + std::to_string(REACH_MAX_E);
        return SMX_ERR_ARG;
    }
    std::vector<uint32_t> order;
    P.jobs.resize(n_jobs);
    for (uint32_t j = 0; j < n_jobs; j++) {
        const smx_reach_job &J = jobs[j];
        if ((uint64_t)J.q0 + J.nq > n_seqs || (uint64_t)J.t0 + J.nt > n_seqs) {
            *why = "job " + std::to_string(j) + ": query or target range out of bounds";
            return SMX_ERR_ARG;
        }
        if (J.nq) order.push_back(j);
        P.jobs[j] = ReachJobDev{J.q0, J.nq, J.t0, J.nt, P.n_rows, P.n_pairs};
        P.n_rows += J.nq;
        P.n_pairs += (uint64_t)J.nq * J.nt;
    }
    // the query ranges may not overlap: every query has one row of keys.  Target ranges may: many jobs over one pool
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return jobs[a].q0 < jobs[b].q0; });
    for (size_t i = 1; i < order.size(); i++)
        if ((uint64_t)jobs[order[i - 1]].q0 + jobs[order[i - 1]].nq > jobs[order[i]].q0) {
            *why = "jobs " + std::to_string(order[i - 1]) + " and " + std::to_string(order[i]) + ": query ranges overlap";
            return SMX_ERR_ARG;
        }
    P.len.assign(n_seqs, 0);
    std::vector<int32_t> cover((size_t)n_seqs + 1, 0);     // +1 / -1 at the ends of every query and target range
    for (uint32_t j = 0; j < n_jobs; j++) {
        const smx_reach_job &J = jobs[j];
        if (J.nq) { cover[J.q0]++; cover[(size_t)J.q0 + J.nq]--; }
        if (J.nt) { cover[J.t0]++; cover[(size_t)J.t0 + J.nt]--; }
    }
    int32_t depth = 0;
    for (uint32_t r = 0; r < n_seqs; r++) {
        if (off[r + 1] < off[r]) {
            *why = "sequence " + std::to_string(r) + ": bad offsets";
            return SMX_ERR_ARG;
        }
        if (off[r + 1] - off[r] > (uint64_t)REACH_MAX_LEN) {
            *why = "sequence " + std::to_string(r) + ": longer than 2^30 - 1 bytes";
            return SMX_ERR_UNSUPPORTED;
        }
        P.len[r] = (int32_t)(off[r + 1] - off[r]);
        depth += cover[r];
        if (depth > 0 && P.len[r] == 0) {
            *why = "sequence " + std::to_string(r) + ": an empty query or target";
            return SMX_ERR_ARG;
        }
    }
    for (uint32_t j = 0; j < n_jobs; j++) {
        const smx_reach_job &J = jobs[j];
        if (!J.nq || !J.nt) continue;
        const uint64_t per_query = ((uint64_t)J.nt + REACH_CHUNK - 1) / REACH_CHUNK;
        if (P.chunk_start.empty()) P.chunk_start.push_back(0);
        for (uint32_t i = 0; i < J.nq; i++) {
            P.recs.push_back(ReachRec{j, J.q0 + i});
            P.chunks += per_query;
            P.chunk_start.push_back(P.chunks);
        }
    }
    const ChunkGrid G = chunk_grid(P.chunks, REACH_BLOCK_CHUNKS, CHUNK_GRID_MAX);
    P.per_block = G.per_block;
    P.grid = G.grid;
    P.n_keys = P.n_rows * 2 * (E + 1) * REACH_SLOTS;
    P.n_values = P.n_pairs * 2 * (E + 1);
    return SMX_OK;
}

// The sequences as the kernel reads them: sequence s forwards at index s and reversed at index n_seqs + s of one padded
// copy (chunk_padded_sequences: 16-byte aligned, 16 bytes of slack at the end), so that the right side is the left side's code
// over other bytes.  doff receives 2 n_seqs offsets.
inline int reach_sequences(const char *seqs, const uint64_t *off, uint32_t n_seqs, std::vector<uint64_t> *doff,
                           std::vector<unsigned char> *pad, std::string *why) {
    if ((uint64_t)n_seqs * 2 > (uint64_t)UINT32_MAX) {
        *why = "more than 2^31 sequences";
        return SMX_ERR_UNSUPPORTED;
    }
    const uint64_t total = off[n_seqs] - off[0];
    std::vector<char> both((size_t)total * 2 + 1);
    std::vector<uint64_t> off2((size_t)n_seqs * 2 + 1);
    if (total) memcpy(both.data(), seqs + off[0], (size_t)total);
    for (uint32_t s = 0; s < n_seqs; s++) {
        off2[s] = off[s] - off[0];
        off2[(size_t)n_seqs + s] = total + (off[s] - off[0]);
        std::reverse_copy(seqs + off[s], seqs + off[s + 1], both.data() + total + (off[s] - off[0]));
    }
    off2[(size_t)n_seqs * 2] = total * 2;
    std::vector<int32_t> len2;
    return chunk_padded_sequences(both.data(), off2.data(), n_seqs * 2, doff, &len2, pad, why);
}

}  // namespace smx

#endif  // SMX_REACH_PLAN_H
