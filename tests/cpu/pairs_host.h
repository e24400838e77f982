// The clusters kernel (specimux_amd/csrc/smx_pairs.hip) as a host loop over a planned call, shared by the CPU simulation
// (tests/cpu/pairs_plan_sim.cpp) and the sanitizer driver (tests/asan/pairs_driver.cpp).  It walks the plan
// (smx_pairs_plan.h) the way the launches do -- class after class, workgroup after workgroup, each over its chunks
// [b * per_block, (b + 1) * per_block), the first row found by chunk_owner's 64-lane search, the Peq table rebuilt when
// the row's read changes -- and calls pairs_pair exactly as the kernel does.  Neighbours mode emulates one ballot per 64
// lanes with the kernel's two guarded word stores.  Every buffer is a heap allocation of its own of exactly the planned
// size, indexed by the kernel's own expressions.
#ifndef SMX_TESTS_PAIRS_HOST_H
#define SMX_TESTS_PAIRS_HOST_H
#include <cstring>
#include <vector>

#include "chunk_owner_host.h"
#include "nearest_host.h"   // NearestHostTable
#include "smx_pairs_plan.h"

namespace smx {

struct PairsHostCounts {
    long long pairs = 0, chunks = 0, builds = 0, blocks = 0, rows = 0;
    long long rows_late = 0;            // rows whose first chunk is not chunk 0 of the job
    long long word_stores = 0, words_guarded = 0;   // neighbours mode: words stored, words the guards held back
    long long blocks_inside = 0, owner_rounds_max = 0;
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
    std::vector<u64> scratch(P.scratch_words);
    if (out_words->size() != P.n_out) host_twin_fail("the output is not of the planned size");
    uint32_t *out = out_words->data();
    const bool DIST = P.distances;
    size_t rat = 0, cat = 0;
    NearestHostTable T;
    for (int c = 0; c < 6; c++) {
        const uint32_t n_rows = P.n_rows[c];
        if (!n_rows) continue;
        const std::vector<PairsRow> rows(P.rows.begin() + rat, P.rows.begin() + rat + n_rows);
        const std::vector<uint64_t> chunk_start(P.chunk_start.begin() + cat, P.chunk_start.begin() + cat + n_rows + 1);
        rat += n_rows;
        cat += (size_t)n_rows + 1;
        const uint64_t per_block = P.per_block[c], n_chunks = chunk_start[n_rows];
        if (n_chunks != P.chunks[c] || P.grid[c] * per_block < n_chunks) host_twin_fail("the grid does not cover the class's chunks");
        if (counts) counts->rows += n_rows;
        for (uint64_t block = 0; block < P.grid[c]; block++) {
            const uint64_t lo = block * per_block, hi = lo + per_block < n_chunks ? lo + per_block : n_chunks;
            if (lo >= n_chunks) host_twin_fail("a workgroup without chunks");
            int rounds = 0;
            uint32_t p = chunk_owner_host(chunk_start.data(), n_rows, lo, &rounds);
            uint32_t cur_q = 0xffffffffu;
            if (counts) {
                counts->blocks++;
                counts->blocks_inside += chunk_start[p] < lo;
                counts->owner_rounds_max = std::max<long long>(counts->owner_rounds_max, rounds);
            }
            for (uint64_t v = lo; v < hi; v++) {
                while (chunk_start[p + 1] <= v) p++;
                if (chunk_start[p + 1] <= chunk_start[p]) host_twin_fail("a row without chunks");
                const PairsRow R = rows[p];
                const PairsJobDev J = jobs[R.job];
                const uint32_t i = R.read - J.r0;
                const uint32_t c0 = ((i + 1) / MINE_THREADS + (uint32_t)(v - chunk_start[p])) * MINE_THREADS;
                const int m = len[R.read];
                const int W = (m + 63) >> 6, Wp = W | 1;
                if (counts) {
                    counts->chunks++;
                    if (v == chunk_start[p] && (i + 1) / MINE_THREADS > 0) counts->rows_late++;
                }
                if (R.read != cur_q) {
                    T.build(bytes + off[R.read], m, Wp, P.lds_max[c]);
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
                        u64 *sbase = scratch.data() + (size_t)block * 3 * P.words_max0 * MINE_THREADS;   // chunk_lane_state
                        const unsigned char *tb = bytes + off[tj];
                        const int n = len[tj], sw = P.words_max0;
                        switch (CHUNK_CLASS_WORDS[c]) {
                            case 1: d = pairs_host_pair<1>(T, m, W, Wp, k, tb, n, sbase, sw, lane); break;
                            case 2: d = pairs_host_pair<2>(T, m, W, Wp, k, tb, n, sbase, sw, lane); break;
                            case 4: d = pairs_host_pair<4>(T, m, W, Wp, k, tb, n, sbase, sw, lane); break;
                            case 8: d = pairs_host_pair<8>(T, m, W, Wp, k, tb, n, sbase, sw, lane); break;
                            case 16: d = pairs_host_pair<16>(T, m, W, Wp, k, tb, n, sbase, sw, lane); break;
                            default: d = pairs_host_pair<0>(T, m, W, Wp, k, tb, n, sbase, sw, lane); break;
                        }
                        if (counts) { counts->pairs++; counts->class_pairs[c]++; }
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
            }
        }
    }
}

}  // namespace smx

#endif  // SMX_TESTS_PAIRS_HOST_H
