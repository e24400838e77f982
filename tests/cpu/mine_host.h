// The specimine kernel (specimux_amd/csrc/smx_mine.hip) as a host loop over a planned call, shared by the CPU
// simulation (tests/cpu/mine_plan_sim.cpp) and the sanitizer driver (tests/asan/mine_driver.cpp). It walks the plan
// (smx_mine_plan.h) the way the launches do (chunk_walk_host.h), the Peq table rebuilt when the query changes, and
// calls mine_pair / mine_identity exactly as the kernel does. Every buffer is a heap allocation of its own of exactly
// the planned size, indexed by the kernel's own expressions, so a caller under a sanitizer finds any index the plan did
// not budget for.
#ifndef SMX_TESTS_MINE_HOST_H
#define SMX_TESTS_MINE_HOST_H
#include <cstring>
#include <vector>

#include "chunk_walk_host.h"
#include "nearest_host.h"   // NearestHostTable: the Peq table as mine_build_peq leaves it, in the LDS bytes of the launch
#include "smx_mine_plan.h"

namespace smx {

struct MineHostCounts : ChunkWalkCounts {
    long long pairs = 0, builds = 0;
    long long class_pairs[6] = {0, 0, 0, 0, 0, 0};
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
    std::vector<MinePair> pairs;           // the records of the class being walked, an allocation of exactly its n entries
    int cls = -1;
    const ChunkLaunches &L = P;
    std::vector<u64> scratch(L.scratch_words);
    if (distances ? out_dist->size() != P.n_dist : out_best->size() != P.n_best) host_twin_fail("the output is not of the planned size");
    int32_t *dist = distances ? out_dist->data() : nullptr;
    u64 *best = distances ? nullptr : out_best->data();
    NearestHostTable T;
    uint32_t cur_q = 0xffffffffu;
    chunk_walk_host(L, counts, [&](const ChunkStep &S) {
        if (S.c != cls) {
            pairs = std::vector<MinePair>(P.pairs.begin() + S.rec_at, P.pairs.begin() + S.rec_at + P.n[S.c]);
            cls = S.c;
        }
        const MinePair R = pairs[S.p];
        const MineJobDev J = jobs[R.job];
        const uint32_t c0 = (uint32_t)S.at * MINE_THREADS;
        const uint64_t q0 = qoff[R.q];
        const int m = (int)(qoff[R.q + 1] - q0);
        const int W = (m + 63) >> 6, Wp = W | 1;
        if (S.first || R.q != cur_q) {
            T.build(qbytes.data() + q0, m, Wp, L.lds_max[S.c]);
            cur_q = R.q;
            if (counts) counts->builds++;
        }
        for (unsigned lane = 0; lane < MINE_THREADS; lane++) {
            if (!((uint64_t)c0 + lane < J.nt)) continue;
            const uint32_t ti = J.t0 + c0 + lane;
            u64 *sbase = scratch.data() + (size_t)S.block * 3 * L.words_max0 * MINE_THREADS;   // chunk_lane_state
            const unsigned char *tb = tbytes + toff[ti];
            const int n = tlen[ti], sw = L.words_max0;
            const int d = chunk_with_wr(S.wr, [&](auto WR) { return mine_host_pair<WR>(T, m, W, Wp, R.k, tb, n, sbase, sw, lane); });
            if (counts) { counts->pairs++; counts->class_pairs[S.c]++; }
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
    });
}

}  // namespace smx

#endif  // SMX_TESTS_MINE_HOST_H
