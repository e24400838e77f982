// The crosstalk kernel (specimux_amd/csrc/smx_nearest.hip) as a host loop over a planned call, shared by the CPU
// simulation (tests/cpu/nearest_sim.cpp) and the sanitizer driver (tests/asan/nearest_driver.cpp). It walks the plan
// (smx_nearest_plan.h) the way the launches do (chunk_walk_host.h), a chunk over the refs of its run with the Peq table
// rebuilt per ref, and calls pairs_pair and smx_nearest_core.h exactly as the kernel does: two keys per lane for the
// run, then a minimum into the output. Every buffer is indexed by the kernel's own expressions, so a caller that sizes
// them by the plan finds any index the plan did not budget for.
#ifndef SMX_TESTS_NEAREST_HOST_H
#define SMX_TESTS_NEAREST_HOST_H
#include <cstring>
#include <vector>

#include "chunk_walk_host.h"
#include "smx_nearest_plan.h"

namespace smx {

// the sequences as the library uploads them: 16-byte aligned copies, 16 bytes of slack behind the last
struct NearestHostSeqs {
    std::vector<mine_u4> pad;
    std::vector<uint64_t> doff;
    const unsigned char *bytes() const { return reinterpret_cast<const unsigned char *>(pad.data()); }
    NearestHostSeqs(const char *seqs, const uint64_t *off, uint32_t n_seqs) {
        uint64_t at = 0;
        doff.assign(n_seqs, 0);
        for (uint32_t i = 0; i < n_seqs; i++) {
            doff[i] = at;
            at += (off[i + 1] - off[i] + 15) & ~(uint64_t)15;
        }
        pad.assign((size_t)(at / 16 + 1), mine_u4{0, 0, 0, 0});
        unsigned char *b = reinterpret_cast<unsigned char *>(pad.data());
        for (uint32_t i = 0; i < n_seqs; i++) memcpy(b + doff[i], seqs + off[i], (size_t)(off[i + 1] - off[i]));
    }
};

// a ref's Peq table as mine_build_peq leaves it in LDS, in a buffer of the LDS bytes the plan asked for
struct NearestHostTable {
    unsigned short rowmap[256];
    std::vector<u64> peq;
    void build(const unsigned char *q, int m, int Wp, size_t lds_bytes) {
        bool present[256] = {false};
        for (int i = 0; i < m; i++) present[q[i]] = true;
        int base = 1;
        for (int c = 0; c < 256; c++) rowmap[c] = present[c] ? (unsigned short)base++ : (unsigned short)0;
        peq.assign(lds_bytes / 8 - MINE_LDS_HEAD, 0ull);       // what is left of the launch's LDS behind the head
        for (int i = 0; i < base * Wp; i++) peq.at(i) = 0ull;  // the words the kernel clears: inside the request
        for (int i = 0; i < m; i++) peq.at((size_t)rowmap[q[i]] * Wp + (i >> 6)) |= 1ull << (i & 63);
    }
};

struct NearestHostCounts : ChunkWalkCounts {
    long long pairs = 0, builds = 0, mins = 0, runs_of_one = 0, runs_of_class = 0, runs_between = 0;
    long long class_pairs[6] = {0, 0, 0, 0, 0, 0};
};

template <int WR>
inline int nearest_host_pair(const NearestHostTable &T, int m, int W, int Wp, int k, const unsigned char *t, int n, u64 *sbase,
                             int scratch_words, unsigned lane) {
    return mine_lane_state<WR>(sbase, scratch_words, lane, [&](auto &st) {
        return pairs_pair<WR>(st, T.peq.data(), T.rowmap, m, W, Wp, k, t, n);
    });
}

// One call.  dist != nullptr: distances mode (own / other unused); else own / other hold P.n_best keys each, filled with
// NEAREST_NONE by the caller.  scratch: P.scratch_words words.
inline void nearest_host_run(const NearestPlan &P, const NearestHostSeqs &seqs, const int32_t *klim, const uint32_t *group,
                             u64 *own, u64 *other, int32_t *dist, u64 *scratch, NearestHostCounts *counts) {
    const unsigned char *bytes = seqs.bytes();
    const int32_t *len = P.len.data();
    const ChunkLaunches &L = P;
    size_t ref_at[CHUNK_CLASSES] = {0, 0, 0, 0, 0, 0};     // every class's own ref list, one after the other
    for (int c = 1; c < CHUNK_CLASSES; c++) ref_at[c] = ref_at[c - 1] + P.n_refs[c - 1];
    NearestHostTable T;
    chunk_walk_host(L, counts, [&](const ChunkStep &S) {
        const int c = S.c;
        const uint32_t *refs = P.refs.data() + ref_at[c];
        const NearestRun R = P.runs[S.rec_at + S.p];
        const NearestJobDev J = P.jobs[R.job];
        NearestKeys K[MINE_THREADS];
        if (counts && S.at == 0) {
            const uint32_t whole = (uint32_t)(std::lower_bound(refs, refs + P.n_refs[c], J.q0 + J.nq) -
                                              std::lower_bound(refs, refs + P.n_refs[c], J.q0));
            if (R.n == whole) counts->runs_of_class++;
            if (R.n == 1) counts->runs_of_one++;
            if (R.n > 1 && R.n < whole) counts->runs_between++;
        }
        for (uint32_t x = 0; x < R.n; x++) {
            const uint32_t ref = refs[R.first + x];
            const int m = len[ref];
            const int W = (m + 63) >> 6, Wp = W | 1;
            T.build(bytes + seqs.doff[ref], m, Wp, L.lds_max[c]);
            if (counts) counts->builds++;
            for (unsigned lane = 0; lane < MINE_THREADS; lane++) {
                const uint32_t ti = (uint32_t)S.at * MINE_THREADS + lane;
                if (!(ti < J.nt)) continue;
                const uint32_t t = J.t0 + ti;
                const int kt = klim[t], n = len[t], sw = L.words_max0;
                const unsigned char *tb = bytes + seqs.doff[t];
                const int k = nearest_limit(klim[ref], kt);
                u64 *sbase = scratch + (size_t)S.block * 3 * L.words_max0 * MINE_THREADS;
                const int d = chunk_with_wr(S.wr, [&](auto WR) { return nearest_host_pair<WR>(T, m, W, Wp, k, tb, n, sbase, sw, lane); });
                if (counts) { counts->pairs++; counts->class_pairs[c]++; }
                if (dist) dist[J.dist_off + (uint64_t)(ref - J.q0) * J.nt + ti] = d;
                else nearest_offer(K[lane], group[ref] == group[t], d, ref);
            }
        }
        if (!dist)
            for (unsigned lane = 0; lane < MINE_THREADS; lane++) {
                const uint32_t ti = (uint32_t)S.at * MINE_THREADS + lane;
                if (!(ti < J.nt)) continue;
                if (K[lane].own != NEAREST_NONE) {     // the kernel's atomicMin
                    u64 &o = own[J.best_off + ti];
                    if (K[lane].own < o) o = K[lane].own;
                    if (counts) counts->mins++;
                }
                if (K[lane].other != NEAREST_NONE) {
                    u64 &o = other[J.best_off + ti];
                    if (K[lane].other < o) o = K[lane].other;
                    if (counts) counts->mins++;
                }
            }
    });
}

}  // namespace smx

#endif  // SMX_TESTS_NEAREST_HOST_H
