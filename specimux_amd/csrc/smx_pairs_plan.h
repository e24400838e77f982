// smx_pairs_plan.h -- the host-side plan of one smx_pairs_* call (smx_calls.cpp): argument checks, the padded reads, the
// jobs with their output offsets, the rows by state class with their chunk prefix, the grids and the scratch size of
// the generic class, and the mirror of the adjacency triangle.  Host only and free of HIP calls, so
// that the CPU simulation (tests/cpu/pairs_plan_sim.cpp) and the sanitizer driver (tests/asan/pairs_driver.cpp) run it
// as it is.
#ifndef SMX_PAIRS_PLAN_H
#define SMX_PAIRS_PLAN_H
#include <algorithm>
#include <string>
#include <vector>

#include "smx_chunk_plan.h"

namespace smx {

constexpr uint64_t PAIRS_BLOCK_CHUNKS = 8;     // chunks a workgroup takes in a row: specimine's, DESIGN.md §10

struct PairsPlan : ChunkLaunches {    // the launch table: the rows per class (n), chunk_start, the grids, the scratch
    bool distances = true;                 // the mode the output was planned for
    std::vector<uint64_t> doff;            // the reads as the kernel reads them (chunk_padded_sequences)
    std::vector<int32_t> len;
    std::vector<unsigned char> pad;
    std::vector<PairsJobDev> jobs;         // the caller's jobs in the caller's order, with their output offsets
    std::vector<PairsRow> rows;            // class after class (0 = generic, 1..5 = 1..16 words), in read order within a class
    // 32-bit words of the output: per job n (n - 1) / 2 distances, or n x ceil(n / 32) adjacency words (a job of one
    // read has a zero word, and no row)
    uint64_t n_out = 0;
};

// The plan of a call.  scratch_budget: the bytes the generic class's state may take (CHUNK_SCRATCH_BYTES in
// production).  Returns SMX_OK, or the status to fail with and why.
inline int pairs_plan(bool distances, const char *reads, const uint64_t *roff, uint32_t n_reads, const smx_pairs_job *jobs,
                      uint32_t n_jobs, uint64_t scratch_budget, PairsPlan *plan, std::string *why) {
    PairsPlan &P = *plan;
    P = PairsPlan();
    P.distances = distances;
    std::vector<size_t> qlds;
    std::vector<int> qclass;
    int rc = chunk_pattern_classes(reads, roff, n_reads, true, &qlds, &qclass, why);
    if (rc != SMX_OK) return rc;
    rc = chunk_padded_sequences(reads, roff, n_reads, &P.doff, &P.len, &P.pad, why);
    if (rc != SMX_OK) return rc;
    // the jobs' ranges may not overlap: every read is a row of at most one matrix
    std::vector<uint32_t> order;
    for (uint32_t j = 0; j < n_jobs; j++) {
        if ((uint64_t)jobs[j].r0 + jobs[j].n > n_reads) {
            *why = "job " + std::to_string(j) + ": read range out of bounds";
            return SMX_ERR_ARG;
        }
        if (jobs[j].n) order.push_back(j);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return jobs[a].r0 < jobs[b].r0; });
    for (size_t i = 1; i < order.size(); i++)
        if ((uint64_t)jobs[order[i - 1]].r0 + jobs[order[i - 1]].n > jobs[order[i]].r0) {
            *why = "jobs " + std::to_string(order[i - 1]) + " and " + std::to_string(order[i]) + " overlap";
            return SMX_ERR_ARG;
        }
    // jobs -> rows with at least one j > i, grouped by the register class of the row's read, in read order
    P.jobs.resize(n_jobs);
    std::vector<PairsRow> rows[6];
    for (uint32_t j = 0; j < n_jobs; j++) {
        const uint64_t n = jobs[j].n;
        P.jobs[j] = PairsJobDev{jobs[j].r0, jobs[j].n, P.n_out};
        P.n_out += distances ? n * (n - (n ? 1 : 0)) / 2 : n * ((n + 31) / 32);
        for (uint32_t i = 0; i + 1 < n; i++) {
            const uint32_t r = jobs[j].r0 + i;
            const int c = qclass[r];
            P.note(c, qlds[r], (size_t)(P.len[r] + 63) / 64);
            rows[c].push_back(PairsRow{j, r});
        }
    }
    for (int c = 0; c < 6; c++) {
        for (const PairsRow &R : rows[c]) {
            // the row's first chunk is the one that holds j = i + 1; chunks are aligned in j
            const uint32_t n = P.jobs[R.job].n, i = R.read - P.jobs[R.job].r0;
            P.append(c, ((uint64_t)n + MINE_THREADS - 1) / MINE_THREADS - (i + 1) / MINE_THREADS);
        }
        P.rows.insert(P.rows.end(), rows[c].begin(), rows[c].end());
    }
    P.seal(PAIRS_BLOCK_CHUNKS, scratch_budget);
    return SMX_OK;
}

// Neighbours mode: the kernel leaves the upper triangle of every job's n x ceil(n / 32) matrix in out; this sets bit i
// of row j for every bit j > i of row i.
inline void pairs_mirror(const PairsPlan &P, uint32_t *out) {
    for (const PairsJobDev &J : P.jobs) {
        const uint32_t nw = (J.n + 31) / 32;
        uint32_t *adj = out + J.out_off;
        for (uint32_t i = 0; i < J.n; i++)
            for (uint32_t w = i / 32; w < nw; w++) {
                uint32_t bits = adj[(size_t)i * nw + w];
                if (w == i / 32) bits &= i % 32 == 31 ? 0u : ~0u << (i % 32 + 1);   // the bits right of the diagonal
                for (; bits; bits &= bits - 1)
                    adj[(size_t)(w * 32 + (uint32_t)__builtin_ctz(bits)) * nw + i / 32] |= 1u << (i % 32);
            }
    }
}

}  // namespace smx

#endif  // SMX_PAIRS_PLAN_H
