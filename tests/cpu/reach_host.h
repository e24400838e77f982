// The bimera kernel (specimux_amd/csrc/smx_reach.hip) as a host loop over a planned call, shared by the CPU simulation
// (tests/cpu/reach_sim.cpp) and the sanitizer driver (tests/asan/reach_driver.cpp).  It walks the plan
// (smx_reach_plan.h) the way the launch does -- workgroup after workgroup, each over its chunks
// [b * per_block, (b + 1) * per_block), a chunk's (target, side) items dealt to the four groups, a group's 32 lanes one
// diagonal each -- and calls smx_reach_core.h exactly as the kernel does; a shuffle is an index into the group's array.
// Every buffer is indexed by the kernel's own expressions, so a caller that sizes them by the plan finds any index the
// plan did not budget for.
#ifndef SMX_TESTS_REACH_HOST_H
#define SMX_TESTS_REACH_HOST_H
#include <cstring>
#include <vector>

#include "chunk_owner_host.h"
#include "smx_reach_plan.h"

namespace smx {

struct ReachHostCounts {
    long long chunks = 0, items = 0, not_eligible = 0, steps = 0, slides = 0, early = 0, inserts = 0, atomics = 0, prechecked = 0;
    long long side_items[2] = {0, 0}, group_items[MINE_THREADS / REACH_LANES] = {0, 0, 0, 0};
    long long slide_q_mod8[8] = {0, 0, 0, 0, 0, 0, 0, 0}, slide_r_mod8[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // where slides start
};

struct ReachHostMin {    // the simulation's "atomic minimum that returns the old value"
    long long *calls;
    u64 operator()(u64 *p, u64 v) const {
        const u64 old = *p;
        if (v < old) *p = v;
        if (calls) ++*calls;
        return old;
    }
};

// the sequences as the library uploads them: forwards, then reversed, in a buffer of exactly the planned size
struct ReachHostSeqs {
    std::vector<unsigned char> pad;
    std::vector<uint64_t> doff;
    int rc;
    std::string why;
    ReachHostSeqs(const char *seqs, const uint64_t *off, uint32_t n_seqs) { rc = reach_sequences(seqs, off, n_seqs, &doff, &pad, &why); }
};

// what one group of 32 lanes does for one (pair, side): out[0 .. E] = reach(e)
inline void reach_host_pair(const unsigned char *qs, int n, const unsigned char *rs, int m, int E, int *out, ReachHostCounts *counts) {
    int fr[REACH_LANES], next[REACH_LANES];
    auto group_max = [&]() {
        int x = fr[0];
        for (int l = 1; l < REACH_LANES; l++) x = reach_max(x, fr[l]);
        return x;
    };
    for (int lane = 0; lane < REACH_LANES; lane++) fr[lane] = lane - E == 0 ? reach_slide(qs, n, rs, m, 0, 0) : REACH_NEG;
    int best = group_max();
    out[0] = best;
    int e = 1;
    for (; e <= E && best < n; e++) {
        for (int lane = 0; lane < REACH_LANES; lane++) {
            const int d = lane - E;
            const int below = lane == 0 ? REACH_NEG : fr[lane - 1], above = lane == REACH_LANES - 1 ? REACH_NEG : fr[lane + 1];
            int f = reach_step(fr[lane], below, above, d, n, m);
            if (f >= 0) {
                if (counts) { counts->slides++; counts->slide_q_mod8[f & 7]++; counts->slide_r_mod8[(f + d) & 7]++; }
                f = reach_slide(qs, n, rs, m, f, f + d);
            }
            next[lane] = f;
        }
        memcpy(fr, next, sizeof fr);
        best = group_max();
        out[e] = best;
        if (counts) counts->steps++;
    }
    if (counts && e <= E) counts->early++;
    for (; e <= E; e++) out[e] = best;
}

// One call.  values != nullptr: matrix mode (keys unused), values holds P.n_values entries filled with 0xFF bytes by the
// caller; else keys holds P.n_keys keys filled with HITS_NONE.
inline void reach_host_run(const ReachPlan &P, const ReachHostSeqs &S, uint32_t n_seqs, const uint32_t *weight,
                           const uint32_t *need, int E, u64 *keys, uint32_t *values, ReachHostCounts *counts) {
    const unsigned char *bytes = S.pad.data();
    const int32_t *len = P.len.data();
    const uint32_t n_recs = (uint32_t)P.recs.size();
    if (!n_recs) return;
    const uint64_t *chunk_start = P.chunk_start.data();
    const uint64_t per_block = P.per_block, n_chunks = chunk_start[n_recs];
    for (uint64_t block = 0; block < P.grid; block++) {
        const uint64_t lo = block * per_block, hi = lo + per_block < n_chunks ? lo + per_block : n_chunks;
        uint32_t p = chunk_owner_host(chunk_start, n_recs, lo);    // the 64-lane search, checked against std::upper_bound
        for (uint64_t v = lo; v < hi; v++) {
            while (chunk_start[p + 1] <= v) p++;
            const ReachRec R = P.recs[p];
            const ReachJobDev J = P.jobs[R.job];
            const uint32_t q = R.query, first = (uint32_t)(v - chunk_start[p]) * REACH_CHUNK;
            const uint32_t count = std::min(REACH_CHUNK, J.nt - first);
            const int n = len[q];
            const uint32_t need_q = need[q];
            if (counts) counts->chunks++;
            for (uint32_t group = 0; group < MINE_THREADS / REACH_LANES; group++)
                for (uint32_t item = group; item < count * 2; item += MINE_THREADS / REACH_LANES) {
                    const uint32_t ti = first + (item >> 1), t = J.t0 + ti;
                    const int side = (int)(item & 1);
                    if (!reach_eligible(q, t, need_q, weight[t])) {
                        if (counts) counts->not_eligible++;
                        continue;
                    }
                    const unsigned char *qs = bytes + S.doff[(size_t)side * n_seqs + q], *rs = bytes + S.doff[(size_t)side * n_seqs + t];
                    int mine[REACH_MAX_E + 1];
                    reach_host_pair(qs, n, rs, len[t], E, mine, counts);
                    if (counts) { counts->items++; counts->side_items[side]++; counts->group_items[group]++; }
                    for (int lane = 0; lane <= E; lane++) {
                        if (values) {
                            values[reach_value_at(J.mat_off + (uint64_t)(q - J.q0) * J.nt + ti, side, lane, E)] = (uint32_t)mine[lane];
                        } else {
                            u64 *slots = keys + reach_slot_at(J.row_off + (q - J.q0), side, lane, E);
                            const u64 key = reach_key((uint32_t)mine[lane], t);
                            if (counts) { counts->inserts++; if (key > slots[REACH_SLOTS - 1]) counts->prechecked++; }
                            hits_insert(slots, REACH_SLOTS, key, ReachHostMin{counts ? &counts->atomics : nullptr});
                        }
                    }
                }
        }
    }
}

}  // namespace smx

#endif  // SMX_TESTS_REACH_HOST_H
