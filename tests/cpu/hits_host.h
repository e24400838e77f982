// The identify kernel (specimux_amd/csrc/smx_hits.hip) as a host loop over a planned call, shared by the CPU simulation
// (tests/cpu/hits_sim.cpp) and the sanitizer driver (tests/asan/hits_driver.cpp). It walks the plan (smx_hits_plan.h)
// the way the launches do (chunk_walk_host.h), the Peq table rebuilt when the pattern changes, a lane's text taken
// through the order array, and calls mine_pair and smx_hits_core.h exactly as the kernel does. Every buffer is indexed
// by the kernel's own expressions, so a caller that sizes them by the plan finds any index the plan did not budget for.
#ifndef SMX_TESTS_HITS_HOST_H
#define SMX_TESTS_HITS_HOST_H
#include <cstring>
#include <vector>

#include "nearest_host.h"   // NearestHostSeqs, NearestHostTable: the padded sequences and the Peq table, as uploaded / built
#include "smx_hits_plan.h"

namespace smx {

struct HitsHostCounts : ChunkWalkCounts {
    long long pairs = 0, builds = 0, inserts = 0, atomics = 0, prechecked = 0, side_pairs[2] = {0, 0};
    long long class_pairs[6] = {0, 0, 0, 0, 0, 0};
};

struct HitsHostMin {     // the simulation's "atomic minimum that returns the old value"
    long long *calls;
    u64 operator()(u64 *p, u64 v) const {
        const u64 old = *p;
        if (v < old) *p = v;
        if (calls) ++*calls;
        return old;
    }
};

template <int WR>
inline int hits_host_pair(const NearestHostTable &T, int m, int W, int Wp, int k, const unsigned char *t, int n, u64 *sbase,
                          int scratch_words, unsigned lane) {
    return mine_lane_state<WR>(sbase, scratch_words, lane, [&](auto &st) {
        return mine_pair<WR>(st, T.peq.data(), T.rowmap, m, W, Wp, k, t, n);
    });
}

// One call.  dist != nullptr: distances mode (keys unused), dist holds P.n_dist entries filled with -1 by the caller;
// else keys holds P.n_rows x K keys filled with HITS_NONE.  scratch: P.scratch_words words.
inline void hits_host_run(const HitsPlan &P, const NearestHostSeqs &seqs, const int32_t *klim, int K, u64 *keys, int32_t *dist,
                          u64 *scratch, HitsHostCounts *counts) {
    const unsigned char *bytes = seqs.bytes();
    const int32_t *len = P.len.data();
    const uint32_t *ord = P.ord.data();
    const ChunkLaunches &L = P;
    NearestHostTable T;
    uint32_t cur = 0xffffffffu;
    chunk_walk_host(L, counts, [&](const ChunkStep &S) {
        const HitsRec R = P.recs[S.rec_at + S.p];
        const HitsJobDev J = P.jobs[R.job];
        const int m = len[R.pattern];
        const int W = (m + 63) >> 6, Wp = W | 1;
        if (S.first || R.pattern != cur) {
            T.build(bytes + seqs.doff[R.pattern], m, Wp, L.lds_max[S.c]);
            cur = R.pattern;
            if (counts) counts->builds++;
        }
        for (unsigned lane = 0; lane < MINE_THREADS; lane++) {
            const uint32_t cc = (uint32_t)S.at * MINE_THREADS + lane;
            if (!(cc < R.n)) continue;
            const uint32_t text = ord[R.first + cc];
            u64 *sbase = scratch + (size_t)S.block * 3 * L.words_max0 * MINE_THREADS;
            const unsigned char *tb = bytes + seqs.doff[text];
            const int k = klim[R.pattern], n = len[text], sw = L.words_max0;
            const int d = chunk_with_wr(S.wr, [&](auto WR) { return hits_host_pair<WR>(T, m, W, Wp, k, tb, n, sbase, sw, lane); });
            if (counts) { counts->pairs++; counts->class_pairs[S.c]++; counts->side_pairs[R.side ? 1 : 0]++; }
            const uint32_t q = (R.side ? text : R.pattern) - J.q0, t = (R.side ? R.pattern : text) - J.t0;
            if (dist) {
                dist[J.dist_off + (uint64_t)q * J.nt + t] = d;
            } else if (d >= 0) {
                u64 *slots = keys + (J.row_off + q) * (uint64_t)K;
                const u64 key = hits_key(d, m, t);
                if (counts) { counts->inserts++; if (key > slots[K - 1]) counts->prechecked++; }
                hits_insert(slots, K, key, HitsHostMin{counts ? &counts->atomics : nullptr});
            }
        }
    });
}

}  // namespace smx

#endif  // SMX_TESTS_HITS_HOST_H
