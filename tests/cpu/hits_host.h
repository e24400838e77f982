// The identify kernel (specimux_amd/csrc/smx_hits.hip) as a host loop over a planned call, shared by the CPU simulation
// (tests/cpu/hits_sim.cpp) and the sanitizer driver (tests/asan/hits_driver.cpp).  It walks the plan (smx_hits_plan.h)
// the way the launches do -- class after class, workgroup after workgroup, each over its chunks
// [b * per_block, (b + 1) * per_block), the Peq table rebuilt when the pattern changes, a lane's text taken through the
// order array -- and calls mine_pair and smx_hits_core.h exactly as the kernel does.  Every buffer is indexed by the
// kernel's own expressions, so a caller that sizes them by the plan finds any index the plan did not budget for.
#ifndef SMX_TESTS_HITS_HOST_H
#define SMX_TESTS_HITS_HOST_H
#include <cstring>
#include <vector>

#include "nearest_host.h"   // NearestHostSeqs, NearestHostTable: the padded sequences and the Peq table, as uploaded / built
#include "smx_hits_plan.h"

namespace smx {

struct HitsHostCounts {
    long long pairs = 0, chunks = 0, builds = 0, inserts = 0, atomics = 0, prechecked = 0, side_pairs[2] = {0, 0};
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
inline void hits_host_run(const HitsPlan &P, const NearestHostSeqs &S, const int32_t *klim, int K, u64 *keys, int32_t *dist,
                          u64 *scratch, HitsHostCounts *counts) {
    const unsigned char *bytes = S.bytes();
    const int32_t *len = P.len.data();
    const uint32_t *ord = P.ord.data();
    size_t rat = 0, cat = 0;
    NearestHostTable T;
    for (int c = 0; c < 6; c++) {
        const uint32_t n_recs = P.n_recs[c];
        if (!n_recs) continue;
        const HitsRec *recs = P.recs.data() + rat;
        const uint64_t *chunk_start = P.chunk_start.data() + cat;
        rat += n_recs;
        cat += (size_t)n_recs + 1;
        const uint64_t per_block = P.per_block[c], n_chunks = chunk_start[n_recs];
        for (uint64_t block = 0; block < P.grid[c]; block++) {
            const uint64_t lo = block * per_block, hi = lo + per_block < n_chunks ? lo + per_block : n_chunks;
            // the record that owns lo, as chunk_owner finds it: the last p with chunk_start[p] <= lo
            uint32_t p = (uint32_t)(std::upper_bound(chunk_start, chunk_start + n_recs, lo) - chunk_start) - 1;
            uint32_t cur = 0xffffffffu;
            for (uint64_t v = lo; v < hi; v++) {
                while (chunk_start[p + 1] <= v) p++;
                const HitsRec R = recs[p];
                const HitsJobDev J = P.jobs[R.job];
                const int m = len[R.pattern];
                const int W = (m + 63) >> 6, Wp = W | 1;
                if (counts) counts->chunks++;
                if (R.pattern != cur) {
                    T.build(bytes + S.doff[R.pattern], m, Wp, P.lds_max[c]);
                    cur = R.pattern;
                    if (counts) counts->builds++;
                }
                for (unsigned lane = 0; lane < MINE_THREADS; lane++) {
                    const uint32_t cc = (uint32_t)(v - chunk_start[p]) * MINE_THREADS + lane;
                    if (!(cc < R.n)) continue;
                    const uint32_t text = ord[R.first + cc];
                    u64 *sbase = scratch + (size_t)block * 3 * P.words_max0 * MINE_THREADS;
                    const unsigned char *tb = bytes + S.doff[text];
                    const int k = klim[R.pattern], n = len[text];
                    int d;
                    switch (CHUNK_CLASS_WORDS[c]) {
                        case 1: d = hits_host_pair<1>(T, m, W, Wp, k, tb, n, sbase, P.words_max0, lane); break;
                        case 2: d = hits_host_pair<2>(T, m, W, Wp, k, tb, n, sbase, P.words_max0, lane); break;
                        case 4: d = hits_host_pair<4>(T, m, W, Wp, k, tb, n, sbase, P.words_max0, lane); break;
                        case 8: d = hits_host_pair<8>(T, m, W, Wp, k, tb, n, sbase, P.words_max0, lane); break;
                        case 16: d = hits_host_pair<16>(T, m, W, Wp, k, tb, n, sbase, P.words_max0, lane); break;
                        default: d = hits_host_pair<0>(T, m, W, Wp, k, tb, n, sbase, P.words_max0, lane); break;
                    }
                    if (counts) { counts->pairs++; counts->class_pairs[c]++; counts->side_pairs[R.side ? 1 : 0]++; }
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
            }
        }
    }
}

}  // namespace smx

#endif  // SMX_TESTS_HITS_HOST_H
