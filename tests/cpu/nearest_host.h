// The crosstalk kernel (specimux_amd/csrc/smx_nearest.hip) as a host loop over a planned call, shared by the CPU
// simulation (tests/cpu/nearest_sim.cpp) and the sanitizer driver (tests/asan/nearest_driver.cpp).  It walks the plan
// (smx_nearest_plan.h) the way the launches do -- class after class, workgroup after workgroup, each over its chunks
// [b * per_block, (b + 1) * per_block), a chunk over the refs of its run with the Peq table rebuilt per ref -- and calls
// pairs_pair and smx_nearest_core.h exactly as the kernel does: two keys per lane for the run, then a minimum into the
// output.  Every buffer is indexed by the kernel's own expressions, so a caller that sizes them by the plan finds any
// index the plan did not budget for.
#ifndef SMX_TESTS_NEAREST_HOST_H
#define SMX_TESTS_NEAREST_HOST_H
#include <cstring>
#include <vector>

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

struct NearestHostCounts {
    long long pairs = 0, chunks = 0, builds = 0, mins = 0, runs_of_one = 0, runs_of_class = 0, runs_between = 0;
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
inline void nearest_host_run(const NearestPlan &P, const NearestHostSeqs &S, const int32_t *klim, const uint32_t *group,
                             u64 *own, u64 *other, int32_t *dist, u64 *scratch, NearestHostCounts *counts) {
    const unsigned char *bytes = S.bytes();
    const int32_t *len = P.len.data();
    size_t qat = 0, rat = 0, cat = 0;
    NearestHostTable T;
    for (int c = 0; c < 6; c++) {
        const uint32_t n_runs = P.n_runs[c];
        const uint32_t *refs = P.refs.data() + qat;
        qat += P.n_refs[c];
        if (!n_runs) continue;
        const NearestRun *runs = P.runs.data() + rat;
        const uint64_t *chunk_start = P.chunk_start.data() + cat;
        rat += n_runs;
        cat += (size_t)n_runs + 1;
        const uint64_t per_block = P.per_block[c], n_chunks = chunk_start[n_runs];
        for (uint64_t block = 0; block < P.grid[c]; block++) {
            const uint64_t lo = block * per_block, hi = lo + per_block < n_chunks ? lo + per_block : n_chunks;
            // the record that owns lo, as chunk_owner finds it: the last p with chunk_start[p] <= lo
            uint32_t p = (uint32_t)(std::upper_bound(chunk_start, chunk_start + n_runs, lo) - chunk_start) - 1;
            for (uint64_t v = lo; v < hi; v++) {
                while (chunk_start[p + 1] <= v) p++;
                const NearestRun R = runs[p];
                const NearestJobDev J = P.jobs[R.job];
                NearestKeys K[MINE_THREADS];
                if (counts) {
                    counts->chunks++;
                    if (v == chunk_start[p]) {
                        const uint32_t whole = (uint32_t)(std::lower_bound(refs, refs + P.n_refs[c], J.q0 + J.nq) -
                                                          std::lower_bound(refs, refs + P.n_refs[c], J.q0));
                        if (R.n == whole) counts->runs_of_class++;
                        if (R.n == 1) counts->runs_of_one++;
                        if (R.n > 1 && R.n < whole) counts->runs_between++;
                    }
                }
                for (uint32_t x = 0; x < R.n; x++) {
                    const uint32_t ref = refs[R.first + x];
                    const int m = len[ref];
                    const int W = (m + 63) >> 6, Wp = W | 1;
                    T.build(bytes + S.doff[ref], m, Wp, P.lds_max[c]);
                    if (counts) counts->builds++;
                    for (unsigned lane = 0; lane < MINE_THREADS; lane++) {
                        const uint32_t ti = (uint32_t)(v - chunk_start[p]) * MINE_THREADS + lane;
                        if (!(ti < J.nt)) continue;
                        const uint32_t t = J.t0 + ti;
                        const int kt = klim[t], n = len[t];
                        const unsigned char *tb = bytes + S.doff[t];
                        const int k = nearest_limit(klim[ref], kt);
                        u64 *sbase = scratch + (size_t)block * 3 * P.words_max0 * MINE_THREADS;
                        int d;
                        switch (CHUNK_CLASS_WORDS[c]) {
                            case 1: d = nearest_host_pair<1>(T, m, W, Wp, k, tb, n, sbase, P.words_max0, lane); break;
                            case 2: d = nearest_host_pair<2>(T, m, W, Wp, k, tb, n, sbase, P.words_max0, lane); break;
                            case 4: d = nearest_host_pair<4>(T, m, W, Wp, k, tb, n, sbase, P.words_max0, lane); break;
                            case 8: d = nearest_host_pair<8>(T, m, W, Wp, k, tb, n, sbase, P.words_max0, lane); break;
                            case 16: d = nearest_host_pair<16>(T, m, W, Wp, k, tb, n, sbase, P.words_max0, lane); break;
                            default: d = nearest_host_pair<0>(T, m, W, Wp, k, tb, n, sbase, P.words_max0, lane); break;
                        }
                        if (counts) { counts->pairs++; counts->class_pairs[c]++; }
                        if (dist) dist[J.dist_off + (uint64_t)(ref - J.q0) * J.nt + ti] = d;
                        else nearest_offer(K[lane], group[ref] == group[t], d, ref);
                    }
                }
                if (!dist)
                    for (unsigned lane = 0; lane < MINE_THREADS; lane++) {
                        const uint32_t ti = (uint32_t)(v - chunk_start[p]) * MINE_THREADS + lane;
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
            }
        }
    }
}

}  // namespace smx

#endif  // SMX_TESTS_NEAREST_HOST_H
