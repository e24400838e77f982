// The clusters kernel (specimux_amd/csrc/smx_pairs.hip) as a host loop over a planned call, shared by the CPU
// simulation (tests/cpu/pairs_plan_sim.cpp) and the sanitizer driver (tests/asan/pairs_driver.cpp). It walks the plan
// (smx_pairs_plan.h) the way the launches do (chunk_walk_host.h), the Peq table rebuilt when the row's read changes,
// and calls pairs_pair exactly as the kernel does. Neighbours mode emulates one ballot per 64 lanes with the kernel's
// two guarded word stores. Every buffer is a heap allocation of its own of exactly the planned size, indexed by the
// kernel's own expressions.
#ifndef SMX_TESTS_PAIRS_HOST_H
#define SMX_TESTS_PAIRS_HOST_H
#include <cstring>
#include <vector>

#include "chunk_walk_host.h"
#include "nearest_host.h"   // NearestHostTable
#include "smx_pairs_plan.h"

namespace smx {

struct PairsHostCounts : ChunkWalkCounts {   // records: the rows
    long long pairs = 0, builds = 0;
    long long rows_late = 0;            // rows whose first chunk is not chunk 0 of the job
    long long word_stores = 0, words_guarded = 0;   // neighbours mode: words stored, words the guards held back
    long long class_pairs[6] = {0, 0, 0, 0, 0, 0};
};

template <int WR>
inline int pairs_host_pair(const NearestHostTable &T, int m, int W, int Wp, int k, const unsigned char *t, int n, u64 *sbase,
                           int scratch_words, unsigned lane) {
    return mine_lane_state<WR>(sbase, scratch_words, lane, [&](auto &st) {
        return pairs_pair<WR>(st, T.peq.data(), T.rowmap, m, W, Wp, k, t, n);
    });
}

// One call in the plan's mode.  out holds P.n_out words: whatever the caller put there in distances mode, zeroes in
// neighbours mode (as the call zeroes them).  The triangle is not mirrored here (pairs_mirror).
inline void pairs_host_run(const PairsPlan &P, const int32_t *klim_in, uint32_t n_reads, std::vector<uint32_t> *out_words,
                           PairsHostCounts *counts) {
    std::vector<mine_u4> pad(P.pad.size() / 16);
    if (P.pad.size() % 16) host_twin_fail("the padded reads are not whole 16-byte words");
    memcpy(pad.data(), P.pad.data(), P.pad.size());
    const unsigned char *bytes = reinterpret_cast<const unsigned char *>(pad.data());
    const std::vector<uint64_t> off(P.doff);
    const std::vector<int32_t> len(P.len), klim(klim_in, klim_in + n_reads);
    const std::vector<PairsJobDev> jobs(P.jobs);
    std::vector<PairsRow> rows;            // the rows of the class being walked, an allocation of exactly its n entries
    int cls = -1;
    const ChunkLaunches &L = P;
    std::vector<u64> scratch(L.scratch_words);
    if (out_words->size() != P.n_out) host_twin_fail("the output is not of the planned size");
    uint32_t *out = out_words->data();
    const bool DIST = P.distances;
    NearestHostTable T;
    uint32_t cur_q = 0xffffffffu;
    chunk_walk_host(L, counts, [&](const ChunkStep &S) {
        if (S.c != cls) {
            rows = std::vector<PairsRow>(P.rows.begin() + S.rec_at, P.rows.begin() + S.rec_at + P.n[S.c]);
            cls = S.c;
        }
        const PairsRow R = rows[S.p];
        const PairsJobDev J = jobs[R.job];
        const uint32_t i = R.read - J.r0;
        const uint32_t c0 = ((i + 1) / MINE_THREADS + (uint32_t)S.at) * MINE_THREADS;
        const int m = len[R.read];
        const int W = (m + 63) >> 6, Wp = W | 1;
        if (counts && S.at == 0 && (i + 1) / MINE_THREADS > 0) counts->rows_late++;
        if (S.first || R.read != cur_q) {
            T.build(bytes + off[R.read], m, Wp, L.lds_max[S.c]);
            cur_q = R.read;
            if (counts) counts->builds++;
        }
        bool hit[MINE_THREADS];
        for (unsigned lane = 0; lane < MINE_THREADS; lane++) {
            const uint32_t j = c0 + lane;
            const bool active = j > i && j < J.n;
            int d = -1;
            if (active) {
                const uint32_t tj = J.r0 + j;
                const int ki = klim[R.read], kj = klim[tj];
                const int k = (ki < 0 || kj < 0) ? -1 : std::max(ki, kj);
                u64 *sbase = scratch.data() + (size_t)S.block * 3 * L.words_max0 * MINE_THREADS;   // chunk_lane_state
                const unsigned char *tb = bytes + off[tj];
                const int n = len[tj], sw = L.words_max0;
                d = chunk_with_wr(S.wr, [&](auto WR) { return pairs_host_pair<WR>(T, m, W, Wp, k, tb, n, sbase, sw, lane); });
                if (counts) { counts->pairs++; counts->class_pairs[S.c]++; }
            }
            hit[lane] = active && d >= 0;
            if (DIST && active) out[J.out_off + (uint64_t)i * J.n - (uint64_t)i * (i + 1) / 2 + (j - i - 1)] = (uint32_t)d;
        }
        if (!DIST)
            for (unsigned lane = 0; lane < MINE_THREADS; lane += 64) {      // the first lane of each wave
                u64 bal = 0;
                for (unsigned l = 0; l < 64; l++)
                    if (hit[lane + l]) bal |= 1ull << l;
                const uint32_t nw = (J.n + 31) / 32, w0 = (c0 + (lane & 64u)) / 32;
                uint32_t *row = out + J.out_off + (uint64_t)i * nw;
                if (w0 < nw) row[w0] = (uint32_t)bal;
                if (w0 + 1 < nw) row[w0 + 1] = (uint32_t)(bal >> 32);
                if ((!(w0 < nw) && (uint32_t)bal) || (!(w0 + 1 < nw) && (uint32_t)(bal >> 32)))
                    host_twin_fail("a word the guards hold back has a neighbour in it");
                if (counts) {
                    counts->word_stores += (w0 < nw) + (w0 + 1 < nw);
                    counts->words_guarded += !(w0 < nw) + !(w0 + 1 < nw);
                }
            }
    });
}

}  // namespace smx

#endif  // SMX_TESTS_PAIRS_HOST_H
