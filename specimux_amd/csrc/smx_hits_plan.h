// smx_hits_plan.h -- the host-side plan of one smx_best_hits* call (smx_calls.cpp): argument checks, the jobs with
// their offsets, the two orders of every job, the work records by state class with their chunk prefix, the grids and
// the scratch size of the generic class.  Host only and free of HIP calls, so that the CPU simulation
// (tests/cpu/hits_sim.cpp) and the sanitizer driver (tests/asan/hits_driver.cpp) run it as it is.
//
// The eligible texts of every pattern are one contiguous window of an order array:
//   tord  a job's targets sorted by (length, index); side Q: the texts of query q are the targets with
//         len_q <= len <= hits_max_text(len_q)
//   qord  a job's queries sorted by (length, index); side T: the texts of target t are the queries with
//         len_t < len <= hits_max_text(len_t)
// so every eligible pair lies in exactly one window, and a pair that coverage excludes is never launched.
#ifndef SMX_HITS_PLAN_H
#define SMX_HITS_PLAN_H
#include <algorithm>
#include <string>
#include <vector>

#include "smx_chunk_plan.h"
#include "smx_hits_core.h"

namespace smx {

constexpr uint64_t HITS_BLOCK_CHUNKS = 8;                       // chunks a workgroup takes in a row: specimine's, DESIGN.md §10

struct HitsPlan : ChunkLaunches {    // the launch table: the records per class (n), chunk_start, the grids, the scratch
    std::vector<HitsJobDev> jobs;          // the caller's jobs in the caller's order
    std::vector<int32_t> len;              // per sequence
    std::vector<uint32_t> ord;             // job after job its tord, then its qord: sequence indices
    std::vector<HitsRec> recs;             // class after class (0 = generic, 1..5 = 1..16 words), by pattern within a class
    // lds_max is 0 everywhere after a lengths-only call
    uint64_t n_rows = 0, n_dist = 0;       // sum(nq), sum(nq x nt)
    uint64_t n_pairs = 0;                  // sum of the records' n: the pairs the call aligns
};

// The plan of a call.  seqs may be nullptr (a lengths-only call): every check but the LDS one is made, and the records
// are planned, from the offsets alone.  Returns SMX_OK, or the status to fail with and why.
inline int hits_plan(const char *seqs, const uint64_t *off, uint32_t n_seqs, const smx_hits_job *jobs, uint32_t n_jobs,
                     uint32_t K, uint32_t min_cov_permille, HitsPlan *plan, std::string *why) {
    HitsPlan &P = *plan;
    P = HitsPlan();
    if (K < 1 || K > (uint32_t)HITS_MAX_K) {
        *why = "K = " + std::to_string(K) + " outside 1.." + std::to_string(HITS_MAX_K);
        return SMX_ERR_ARG;
    }
    if (min_cov_permille > 1000) {
        *why = "min_cov_permille = " + std::to_string(min_cov_permille) + " outside 0..1000";
        return SMX_ERR_ARG;
    }
    const int cov = (int)min_cov_permille;
    std::vector<uint32_t> order;
    P.jobs.resize(n_jobs);
    for (uint32_t j = 0; j < n_jobs; j++) {
        const smx_hits_job &J = jobs[j];
        if ((uint64_t)J.q0 + J.nq > n_seqs || (uint64_t)J.t0 + J.nt > n_seqs) {
            *why = "job " + std::to_string(j) + ": query or target range out of bounds";
            return SMX_ERR_ARG;
        }
        if ((uint64_t)J.nt > HITS_MAX_TARGETS) {
            *why = "job " + std::to_string(j) + ": " + std::to_string(J.nt) + " targets, more than 2^24";
            return SMX_ERR_UNSUPPORTED;
        }
        if (J.nq) order.push_back(j);
        P.jobs[j] = HitsJobDev{J.q0, J.nq, J.t0, J.nt, P.n_rows, P.n_dist};
        P.n_rows += J.nq;
        P.n_dist += (uint64_t)J.nq * J.nt;
    }
    // the query ranges may not overlap: every query has one row of keys.  Target ranges may: many jobs over one database
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return jobs[a].q0 < jobs[b].q0; });
    for (size_t i = 1; i < order.size(); i++)
        if ((uint64_t)jobs[order[i - 1]].q0 + jobs[order[i - 1]].nq > jobs[order[i]].q0) {
            *why = "jobs " + std::to_string(order[i - 1]) + " and " + std::to_string(order[i]) + ": query ranges overlap";
            return SMX_ERR_ARG;
        }
    P.len.assign(n_seqs, 0);
    std::vector<int32_t> cover((size_t)n_seqs + 1, 0);     // +1 / -1 at the ends of every query and target range
    for (uint32_t j = 0; j < n_jobs; j++) {
        const smx_hits_job &J = jobs[j];
        if (J.nq) { cover[J.q0]++; cover[(size_t)J.q0 + J.nq]--; }
        if (J.nt) { cover[J.t0]++; cover[(size_t)J.t0 + J.nt]--; }
    }
    int32_t depth = 0;
    for (uint32_t r = 0; r < n_seqs; r++) {
        if (off[r + 1] < off[r] || off[r + 1] - off[r] > (uint64_t)INT32_MAX) {
            *why = "sequence " + std::to_string(r) + ": bad offsets";
            return SMX_ERR_ARG;
        }
        P.len[r] = (int32_t)(off[r + 1] - off[r]);
        depth += cover[r];
        if (depth > 0 && P.len[r] == 0) {
            *why = "sequence " + std::to_string(r) + ": an empty query or target";
            return SMX_ERR_ARG;
        }
    }
    // the orders and the records
    const int32_t *len = P.len.data();
    auto by_len = [&](uint32_t a, uint32_t b) { return len[a] != len[b] ? len[a] < len[b] : a < b; };
    std::vector<HitsRec> by_class[6];
    std::vector<signed char> cls(n_seqs, -1);      // per sequence that is a pattern: its class, once the LDS check passed
    auto pattern_class = [&](uint32_t r, int *c_out) -> int {
        if (cls[r] >= 0) { *c_out = cls[r]; return SMX_OK; }
        const int m = len[r];
        if ((int64_t)m >= HITS_MAX_PATTERN) {
            *why = "sequence " + std::to_string(r) + ": a pattern of " + std::to_string(m) + " bytes, 2^19 or more";
            return SMX_ERR_UNSUPPORTED;
        }
        const size_t W = ((size_t)m + 63) / 64;
        const int c = chunk_class(W);
        size_t lds = 0;
        if (seqs) {                                // the LDS its Peq table needs
            const ChunkTable T = chunk_table(seqs + off[r], (uint64_t)m);
            if (!T.fits()) {
                *why = T.refusal("pattern " + std::to_string(r) + ": ");
                return SMX_ERR_UNSUPPORTED;
            }
            lds = T.lds;
        }
        P.note(c, lds, W);
        cls[r] = (signed char)c;
        *c_out = c;
        return SMX_OK;
    };
    for (uint32_t j = 0; j < n_jobs; j++) {
        const smx_hits_job &J = jobs[j];
        if (!J.nq || !J.nt) continue;
        if ((uint64_t)P.ord.size() + J.nq + J.nt > (uint64_t)UINT32_MAX) {
            *why = "job " + std::to_string(j) + ": the order arrays of the call exceed 2^32 entries";
            return SMX_ERR_UNSUPPORTED;
        }
        const uint32_t tbase = (uint32_t)P.ord.size();
        for (uint32_t i = 0; i < J.nt; i++) P.ord.push_back(J.t0 + i);
        std::sort(P.ord.begin() + tbase, P.ord.end(), by_len);
        const uint32_t qbase = (uint32_t)P.ord.size();
        for (uint32_t i = 0; i < J.nq; i++) P.ord.push_back(J.q0 + i);
        std::sort(P.ord.begin() + qbase, P.ord.end(), by_len);
        // [first index with len >= lo_len, first index with len > hi_len) of an order
        auto window = [&](uint32_t base, uint32_t n, int64_t lo_len, int64_t hi_len, uint32_t *first, uint32_t *count) {
            const uint32_t *b = P.ord.data() + base, *e = b + n;
            const uint32_t *lo = std::partition_point(b, e, [&](uint32_t x) { return (int64_t)len[x] < lo_len; });
            const uint32_t *hi = std::partition_point(lo, e, [&](uint32_t x) { return (int64_t)len[x] <= hi_len; });
            *first = (uint32_t)(lo - P.ord.data());
            *count = (uint32_t)(hi - lo);
        };
        for (int side = 0; side < 2; side++) {
            const uint32_t p0 = side ? J.t0 : J.q0, np = side ? J.nt : J.nq;
            for (uint32_t i = 0; i < np; i++) {
                const uint32_t pat = p0 + i;
                const int m = len[pat];
                uint32_t first = 0, n = 0;
                // side Q: targets at least as long as the query; side T: queries longer than the target
                if (side == 0) window(tbase, J.nt, m, hits_max_text(m, cov), &first, &n);
                else window(qbase, J.nq, (int64_t)m + 1, hits_max_text(m, cov), &first, &n);
                if (!n) continue;
                int c = 0;
                const int rc = pattern_class(pat, &c);
                if (rc != SMX_OK) return rc;
                by_class[c].push_back(HitsRec{j, (uint32_t)side, pat, first, n});
                P.n_pairs += n;
            }
        }
    }
    for (int c = 0; c < 6; c++) {
        // one pattern's records next to each other (a target shared by several jobs): its table is built once
        std::stable_sort(by_class[c].begin(), by_class[c].end(), [](const HitsRec &a, const HitsRec &b) { return a.pattern < b.pattern; });
        for (const HitsRec &R : by_class[c]) P.append(c, ((uint64_t)R.n + MINE_THREADS - 1) / MINE_THREADS);
        P.recs.insert(P.recs.end(), by_class[c].begin(), by_class[c].end());
    }
    P.seal(HITS_BLOCK_CHUNKS);
    return SMX_OK;
}

}  // namespace smx

#endif  // SMX_HITS_PLAN_H
