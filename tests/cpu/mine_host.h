// The specimine kernel (specimux_amd/csrc/smx_mine.hip) as a host loop over a planned call, shared by the CPU simulation
// (tests/cpu/mine_plan_sim.cpp) and the sanitizer driver (tests/asan/mine_driver.cpp).  It walks the plan
// (smx_mine_plan.h) the way the launches do -- class after class, workgroup after workgroup, each over its chunks
// [b * per_block, (b + 1) * per_block), the first record found by chunk_owner's 64-lane search, the Peq table rebuilt
// when the query changes -- and calls mine_pair / mine_identity exactly as the kernel does.  Every buffer is a heap
// allocation of its own of exactly the planned size, indexed by the kernel's own expressions, so a caller under a
// sanitizer finds any index the plan did not budget for.
#ifndef SMX_TESTS_MINE_HOST_H
#define SMX_TESTS_MINE_HOST_H
#include <cstring>
#include <vector>

#include "chunk_owner_host.h"
#include "nearest_host.h"   // NearestHostTable: the Peq table as mine_build_peq leaves it, in the LDS bytes of the launch
#include "smx_mine_plan.h"

namespace smx {

struct MineHostCounts {
    long long pairs = 0, chunks = 0, builds = 0, blocks = 0, records = 0;
    long long records_two_chunks = 0;   // records that own more than one chunk
    long long blocks_inside = 0;        // workgroups whose first chunk is not the first of its record
    long long owner_rounds_max = 0;
    long long class_pairs[6] = {0, 0, 0, 0, 0, 0}, class_blocks[6] = {0, 0, 0, 0, 0, 0};
};

template <int WR>
inline int mine_host_pair(const NearestHostTable &T, int m, int W, int Wp, int k, const unsigned char *t, int n, u64 *sbase,
                          int scratch_words, unsigned lane) {
    return mine_lane_state<WR>(sbase, scratch_words, lane, [&](auto &st) {
        return mine_pair<WR>(st, T.peq.data(), T.rowmap, m, W, Wp, k, t, n);
    });
}

// One call.  distances: out_dist holds P.n_dist entries; else out_best holds the P.n_best bit patterns, zeroed by the
// caller as the call zeroes them.  The queries are the caller's bytes as uploaded: qoff[n_queries] of them.
inline void mine_host_run(const MinePlan &P, const char *queries, const uint64_t *qoff_in, uint32_t n_queries, bool distances,
                          std::vector<int32_t> *out_dist, std::vector<u64> *out_best, MineHostCounts *counts) {
    // the uploads, each an allocation of exactly its size
    const std::vector<unsigned char> qbytes(queries, queries + qoff_in[n_queries]);
    const std::vector<uint64_t> qoff(qoff_in, qoff_in + n_queries + 1);
    std::vector<mine_u4> tpad(P.tpad.size() / 16);
    if (P.tpad.size() % 16) host_twin_fail("the padded targets are not whole 16-byte words");
    memcpy(tpad.data(), P.tpad.data(), P.tpad.size());
    const unsigned char *tbytes = reinterpret_cast<const unsigned char *>(tpad.data());
    const std::vector<uint64_t> toff(P.tdoff);
    const std::vector<int32_t> tlen(P.tlen);
    const std::vector<MineJobDev> jobs(P.jobs);
    std::vector<u64> scratch(P.scratch_words);
    if (distances ? out_dist->size() != P.n_dist : out_best->size() != P.n_best) host_twin_fail("the output is not of the planned size");
    int32_t *dist = distances ? out_dist->data() : nullptr;
    u64 *best = distances ? nullptr : out_best->data();
    size_t rat = 0, cat = 0;
    NearestHostTable T;
    for (int c = 0; c < 6; c++) {
        const uint32_t n_pairs = P.n_pairs[c];
        if (!n_pairs) continue;
        // this launch's slice of the record list and of the prefix, as allocations of their own
        const std::vector<MinePair> pairs(P.pairs.begin() + rat, P.pairs.begin() + rat + n_pairs);
        const std::vector<uint64_t> chunk_start(P.chunk_start.begin() + cat, P.chunk_start.begin() + cat + n_pairs + 1);
        rat += n_pairs;
        cat += (size_t)n_pairs + 1;
        const uint64_t per_block = P.per_block[c], n_chunks = chunk_start[n_pairs];
        if (n_chunks != P.chunks[c] || P.grid[c] * per_block < n_chunks) host_twin_fail("the grid does not cover the class's chunks");
        if (counts) {
            counts->records += n_pairs;
            for (uint32_t p = 0; p < n_pairs; p++) counts->records_two_chunks += chunk_start[p + 1] - chunk_start[p] > 1;
        }
        for (uint64_t block = 0; block < P.grid[c]; block++) {
            // chunk_span
            const uint64_t lo = block * per_block, hi = lo + per_block < n_chunks ? lo + per_block : n_chunks;
            if (lo >= n_chunks) host_twin_fail("a workgroup without chunks");
            int rounds = 0;
            uint32_t p = chunk_owner_host(chunk_start.data(), n_pairs, lo, &rounds);
            uint32_t cur_q = 0xffffffffu;
            if (counts) {
                counts->blocks++;
                counts->class_blocks[c]++;
                counts->blocks_inside += chunk_start[p] < lo;
                counts->owner_rounds_max = std::max<long long>(counts->owner_rounds_max, rounds);
            }
            for (uint64_t v = lo; v < hi; v++) {
                while (chunk_start[p + 1] <= v) p++;
                const MinePair R = pairs[p];
                const MineJobDev J = jobs[R.job];
                const uint32_t c0 = (uint32_t)(v - chunk_start[p]) * MINE_THREADS;
                const uint64_t q0 = qoff[R.q];
                const int m = (int)(qoff[R.q + 1] - q0);
                const int W = (m + 63) >> 6, Wp = W | 1;
                if (counts) counts->chunks++;
                if (R.q != cur_q) {
                    T.build(qbytes.data() + q0, m, Wp, P.lds_max[c]);
                    cur_q = R.q;
                    if (counts) counts->builds++;
                }
                for (unsigned lane = 0; lane < MINE_THREADS; lane++) {
                    if (!((uint64_t)c0 + lane < J.nt)) continue;
                    const uint32_t ti = J.t0 + c0 + lane;
                    u64 *sbase = scratch.data() + (size_t)block * 3 * P.words_max0 * MINE_THREADS;   // chunk_lane_state
                    const unsigned char *tb = tbytes + toff[ti];
                    const int n = tlen[ti], sw = P.words_max0;
                    int d;
                    switch (CHUNK_CLASS_WORDS[c]) {
                        case 1: d = mine_host_pair<1>(T, m, W, Wp, R.k, tb, n, sbase, sw, lane); break;
                        case 2: d = mine_host_pair<2>(T, m, W, Wp, R.k, tb, n, sbase, sw, lane); break;
                        case 4: d = mine_host_pair<4>(T, m, W, Wp, R.k, tb, n, sbase, sw, lane); break;
                        case 8: d = mine_host_pair<8>(T, m, W, Wp, R.k, tb, n, sbase, sw, lane); break;
                        case 16: d = mine_host_pair<16>(T, m, W, Wp, R.k, tb, n, sbase, sw, lane); break;
                        default: d = mine_host_pair<0>(T, m, W, Wp, R.k, tb, n, sbase, sw, lane); break;
                    }
                    if (counts) { counts->pairs++; counts->class_pairs[c]++; }
                    if (distances) {
                        dist[J.dist_off + (uint64_t)(R.q - J.q0) * J.nt + c0 + lane] = d;
                    } else {
                        const double identity = mine_identity(d, m, J.min_identity);
                        if (identity > 0.0) {                  // the kernel's atomicMax on the bit pattern
                            u64 bits;
                            memcpy(&bits, &identity, 8);
                            u64 &o = best[J.best_off + c0 + lane];
                            if (bits > o) o = bits;
                        }
                    }
                }
            }
        }
    }
}

}  // namespace smx

#endif  // SMX_TESTS_MINE_HOST_H
