// msa_host.h -- the three kernels of smx_msa.hip as host loops over smx_msa_core.h, thread for thread: the same index
// expressions, the same per-lane state, the same phases and ticks.  Where the kernel lets waves, lanes or threads run in
// any order between two barriers, the loops here visit them in the order the caller asks for (forward, reversed,
// shuffled): the result may not depend on it.  A shuffle is a snapshot of the wave's registers taken before any lane of
// the step changes them.  Shared by tests/cpu/msa_sim.cpp and tests/asan/msa_driver.cpp; msa_host_call runs the plan
// (smx_msa_plan.h) the way msa_call does, over heap blocks of exactly the planned sizes.
#ifndef MSA_HOST_H
#define MSA_HOST_H
#include <algorithm>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "smx_msa_plan.h"

namespace smx {

enum MsaOrder { MSA_FORWARD = 0, MSA_REVERSED = 1, MSA_SHUFFLED = 2 };

struct MsaCounters {
    uint64_t merges = 0, cells = 0, ticks = 0, tiles = 0, steps = 0, edge_ops = 0, launches = 0, words = 0;
};

inline std::vector<uint32_t> msa_visit(uint32_t count, MsaOrder order, std::mt19937 &rng) {
    std::vector<uint32_t> v(count);
    std::iota(v.begin(), v.end(), 0u);
    if (order == MSA_REVERSED) std::reverse(v.begin(), v.end());
    if (order == MSA_SHUFFLED) std::shuffle(v.begin(), v.end(), rng);
    return v;
}

// msa_tips_kernel
inline void msa_host_tips(const unsigned char *bytes, const uint64_t *doff, uint32_t n, const uint64_t *prof_off, MsaCol *prof) {
    for (uint32_t tip = 0; tip < n; tip++) {
        const uint64_t at = doff[tip], len = doff[tip + 1] - at;
        MsaCol *out = prof + prof_off[tip];
        for (uint32_t x = 0; x < MSA_TIPS_THREADS; x++)
            for (uint64_t k = x; k < len; k += MSA_TIPS_THREADS) out[k] = msa_tip_col(bytes[at + k]);
    }
}

// msa_merge_kernel, one workgroup
inline void msa_host_merge(const MsaMergeDev &R, uint32_t X, uint32_t G, MsaCol *prof, uint16_t *maps, uint32_t *tb_all,
                           uint8_t *ops_all, uint64_t *row_all, uint32_t *lens, uint64_t *costs, MsaOrder order,
                           std::mt19937 &rng, MsaCounters *K) {
    const uint32_t La = R.La, Lb = R.Lb, na = R.na, nb = R.nb;
    const MsaCol *pa = prof + R.prof_a, *pb = prof + R.prof_b;
    MsaCol *po = prof + R.prof_out;
    uint32_t *tb = tb_all + R.tb;
    uint8_t *ops = ops_all + R.ops;
    uint64_t *row = row_all + R.row;
    const uint32_t W16 = msa_tb_words(Lb);
    const MsaCol zero = {{0, 0, 0, 0, 0, 0, 0, 0}};
    // ---- 1: forward
    const uint32_t nbands = (La + 63u) / 64u, nsteps = Lb + 63u, nblocks = (nsteps + 63u) / 64u;
    const uint32_t wact = nbands < MSA_WAVES ? nbands : MSA_WAVES;
    const uint32_t ticks = nblocks + MSA_LAG * (wact - 1u);
    struct Lane { MsaCol ca; uint32_t ra, word; uint64_t ga, cur, diagv; };
    for (uint32_t band0 = 0; band0 < nbands; band0 += wact) {
        std::vector<Lane> st(MSA_WAVES * 64u, Lane{zero, 0, 0, 0, 0, 0});
        for (uint32_t tick = 0; tick < ticks; tick++) {
            for (uint32_t wave : msa_visit(MSA_WAVES, order, rng)) {
                const uint32_t band = band0 + wave;
                const bool valid = wave < wact && band < nbands;
                const uint32_t B = tick - MSA_LAG * wave;
                if (!(valid && tick >= MSA_LAG * wave && B < nblocks)) continue;
                Lane *L = &st[wave * 64u];
                if (B == 0) {
                    const uint64_t top0 = band == 0 ? 0 : row[0];
                    uint64_t incl = 0;
                    for (uint32_t lane = 0; lane < 64u; lane++) {   // the scan's result, lane by lane
                        const uint32_t i = band * 64u + lane + 1u;
                        const bool rowok = i <= La;
                        L[lane].ca = rowok ? pa[i - 1u] : zero;
                        L[lane].ra = na - L[lane].ca.c[MSA_GAP];
                        L[lane].ga = rowok ? msa_gap_cost(G, L[lane].ra, nb) : 0;
                        incl += L[lane].ga;
                        L[lane].cur = top0 + incl;
                        L[lane].diagv = L[lane].cur - L[lane].ga;
                        L[lane].word = 0;
                    }
                    row[0] = L[63].cur;
                }
                uint64_t tv[64];
                for (uint32_t lane = 0; lane < 64u; lane++) {
                    const uint32_t c = 64u * B + lane + 1u;
                    tv[lane] = band != 0 && c <= Lb ? row[c] : 0;
                }
                for (uint32_t q = 0; q < 64u; q++) {
                    const uint32_t s = 64u * B + q;
                    if (s >= nsteps) break;
                    uint64_t snap[64];
                    for (uint32_t lane = 0; lane < 64u; lane++) snap[lane] = L[lane].cur;
                    for (uint32_t lane : msa_visit(64u, order, rng)) {
                        const uint32_t i = band * 64u + lane + 1u;
                        const int32_t j = (int32_t)s - (int32_t)lane + 1;
                        if (!(i <= La && j >= 1 && j <= (int32_t)Lb)) continue;
                        const MsaCol cb = pb[j - 1];
                        uint64_t up = lane ? snap[lane - 1u] : 0;
                        const uint32_t rb = nb - cb.c[MSA_GAP];
                        const uint64_t gb = msa_gap_cost(G, rb, na);
                        if (lane == 0) up = band == 0 ? L[lane].diagv + gb : tv[q];
                        uint32_t dir;
                        const uint64_t best = msa_min3(L[lane].diagv + msa_pair_cost(L[lane].ca, L[lane].ra, cb, rb, X, G),
                                                       up + L[lane].ga, L[lane].cur + gb, &dir);
                        L[lane].diagv = up;
                        L[lane].cur = best;
                        const uint32_t jj = (uint32_t)j - 1u;
                        L[lane].word |= dir << (2u * (jj & 15u));
                        if ((jj & 15u) == 15u || (uint32_t)j == Lb) {
                            tb[(uint64_t)(i - 1u) * W16 + (jj >> 4)] = L[lane].word;
                            L[lane].word = 0;
                            if (K) K->words++;
                        }
                        if (lane == 63u) row[j] = best;
                        if (i == La && (uint32_t)j == Lb) costs[R.t] = best;
                        if (K) K->cells++;
                    }
                }
            }
            if (K) K->ticks++;
        }
    }
    // ---- 2: walk back
    uint32_t s_state[3] = {La, Lb, La + Lb};
    std::vector<uint32_t> s_tile(MSA_TILE_ROWS * MSA_TILE_WORDS);
    for (;;) {
        uint32_t i = s_state[0], j = s_state[1];
        if (i == 0 || j == 0) break;
        const uint32_t r0 = i >= MSA_TILE_ROWS ? i - (MSA_TILE_ROWS - 1u) : 1u, wh = (j - 1u) >> 4;
        const uint32_t wl = wh >= MSA_TILE_WORDS - 1u ? wh - (MSA_TILE_WORDS - 1u) : 0u;
        const uint32_t nrows = i - r0 + 1u, nw = wh - wl + 1u;
        std::fill(s_tile.begin(), s_tile.end(), 0xdeadbeefu);      // what the tile held before is not the walk's to read
        for (uint32_t tid : msa_visit(MSA_MERGE_THREADS, order, rng))
            for (uint32_t x = tid; x < nrows * MSA_TILE_WORDS; x += MSA_MERGE_THREADS) {
                const uint32_t r = x / MSA_TILE_WORDS, k = x % MSA_TILE_WORDS;
                if (k < nw) s_tile[x] = tb[(uint64_t)(r0 + r - 1u) * W16 + wl + k];
            }
        uint32_t pos = s_state[2];
        while (i >= r0 && j > 0 && ((j - 1u) >> 4) >= wl) {
            const uint32_t w = s_tile[(i - r0) * MSA_TILE_WORDS + ((j - 1u) >> 4) - wl];
            const uint32_t d = (w >> (2u * ((j - 1u) & 15u))) & 3u;
            ops[--pos] = (uint8_t)d;
            if (d != MSA_LEFT) i--;
            if (d != MSA_UP) j--;
            if (K) K->steps++;
        }
        s_state[0] = i; s_state[1] = j; s_state[2] = pos;
        if (K) K->tiles++;
    }
    const uint32_t ei = s_state[0], ej = s_state[1], epos = s_state[2], edge = ei + ej;
    for (uint32_t tid : msa_visit(MSA_MERGE_THREADS, order, rng))
        for (uint32_t x = tid; x < edge; x += MSA_MERGE_THREADS) ops[epos - 1u - x] = (uint8_t)(ei ? MSA_UP : MSA_LEFT);
    if (K) K->edge_ops += edge;
    // ---- 3: build
    const uint32_t start = epos - edge, len = La + Lb - start, per = msa_chunk(len);
    std::vector<uint32_t> cnt(MSA_MERGE_THREADS), excl(MSA_MERGE_THREADS);
    for (uint32_t tid = 0; tid < MSA_MERGE_THREADS; tid++) {
        const uint32_t p0 = tid * per < len ? tid * per : len, p1 = p0 + per < len ? p0 + per : len;
        uint32_t c = 0;
        for (uint32_t p = p0; p < p1; p++) {
            const uint32_t op = ops[start + p];
            c += (op != MSA_LEFT ? 0x10000u : 0u) + (op != MSA_UP ? 1u : 0u);
        }
        cnt[tid] = c;
    }
    uint32_t run = 0;                                              // the scan's result
    for (uint32_t tid = 0; tid < MSA_MERGE_THREADS; tid++) { excl[tid] = run; run += cnt[tid]; }
    uint16_t *map_a = maps + R.map_a, *map_b = maps + R.map_b;
    for (uint32_t tid : msa_visit(MSA_MERGE_THREADS, order, rng)) {
        const uint32_t p0 = tid * per < len ? tid * per : len, p1 = p0 + per < len ? p0 + per : len;
        uint32_t ia = excl[tid] >> 16, ib = excl[tid] & 0xffffu;
        for (uint32_t p = p0; p < p1; p++) {
            const uint32_t op = ops[start + p];
            const MsaCol a = op != MSA_LEFT ? pa[ia] : zero, b = op != MSA_UP ? pb[ib] : zero;
            po[p] = msa_new_col(op, a, b, na, nb);
            if (op != MSA_LEFT) map_a[ia++] = (uint16_t)p;
            if (op != MSA_UP) map_b[ib++] = (uint16_t)p;
        }
    }
    lens[R.t] = len;
    if (K) K->merges++;
}

// msa_rows_kernel
inline void msa_host_rows(const unsigned char *bytes, const uint64_t *doff, uint32_t n, const uint32_t *parent,
                          const uint64_t *map_off, const uint16_t *maps, uint32_t n_cols, uint8_t *rows, MsaOrder order,
                          std::mt19937 &rng) {
    for (uint32_t tip : msa_visit(n, order, rng)) {
        std::vector<uint8_t> s_row(n_cols, (uint8_t)'-');
        const uint64_t at = doff[tip], len = doff[tip + 1] - at;
        for (uint32_t tid : msa_visit(MSA_ROWS_THREADS, order, rng))
            for (uint64_t k = tid; k < len; k += MSA_ROWS_THREADS) {
                uint32_t col = (uint32_t)k, node = tip;
                for (uint32_t p = parent[node]; p != MSA_NONE; p = parent[node]) {
                    col = maps[map_off[node] + col];
                    node = p;
                }
                if (col < n_cols) s_row[col] = bytes[at + k];
            }
        memcpy(rows + (uint64_t)tip * n_cols, s_row.data(), n_cols);
    }
}

struct MsaHostResult {
    std::vector<uint8_t> rows;        // n x n_cols
    uint32_t n_cols = 0;
    std::vector<uint32_t> lens;
    std::vector<uint64_t> costs;
};

// a heap block of exactly `count` entries (one at least), filled with what an earlier call may have left
template <typename T> T *msa_block(uint64_t count) {
    T *p = new T[count ? count : 1];
    memset((void *)p, 0x7b, (count ? count : 1) * sizeof(T));
    return p;
}

// What smx_msa computes, the way msa_call runs it: every launch over blocks of exactly the planned sizes, the profile
// and map blocks reallocated at their exact new size (and the old content kept) whenever a launch needs more.
inline int msa_host_call(const char *seqs, const uint64_t *off, uint32_t n, const smx_msa_merge *merges, uint32_t X, uint32_t G,
                         uint32_t cap_cols, uint64_t budget, MsaOrder order, uint32_t seed, MsaHostResult *out, MsaCounters *K,
                         std::string *why) {
    MsaPlan P;
    uint8_t rows_probe = 0;
    uint32_t n_cols_probe = 0, lens_probe = 0;
    uint64_t costs_probe = 0;
    const int rc = msa_plan(seqs, off, n, merges, X, G, &rows_probe, &n_cols_probe, &lens_probe, &costs_probe, &P, why);
    if (rc != SMX_OK) return rc;
    out->rows.clear();
    out->n_cols = 0;
    out->lens.assign(P.n_merges, 0);
    out->costs.assign(P.n_merges, 0);
    if (n == 0) return SMX_OK;
    if (n == 1) {
        out->n_cols = (uint32_t)(off[1] - off[0]);
        if (out->n_cols > cap_cols) { *why = "overflow"; return SMX_ERR_OVERFLOW; }
        out->rows.assign(seqs + off[0], seqs + off[1]);
        return SMX_OK;
    }
    std::mt19937 rng(seed);
    MsaState S;
    msa_state_init(P, off, &S);
    std::vector<uint64_t> doff(n + 1);
    for (uint32_t i = 0; i <= n; i++) doff[i] = off[i] - off[0];
    const unsigned char *bytes = (const unsigned char *)seqs + off[0];
    uint64_t prof_cap = S.prof_used, map_cap = 0;
    MsaCol *prof = msa_block<MsaCol>(prof_cap);
    uint16_t *maps = msa_block<uint16_t>(0);
    uint32_t *lens = msa_block<uint32_t>(P.n_merges);
    uint64_t *costs = msa_block<uint64_t>(P.n_merges);
    msa_host_tips(bytes, doff.data(), n, S.prof_off.data(), prof);
    int status = SMX_OK;
    std::vector<MsaLaunch> launches;
    std::vector<MsaMergeDev> recs;
    for (uint32_t v = 1; v <= P.n_levels && status == SMX_OK; v++) {
        msa_level_launches(P, merges, S, v, budget, &launches);
        for (const MsaLaunch &L : launches) {
            msa_launch_records(P, merges, L, &S, &recs);
            if (S.prof_used > prof_cap) {
                MsaCol *bigger = msa_block<MsaCol>(S.prof_used);
                memcpy((void *)bigger, (const void *)prof, prof_cap * sizeof(MsaCol));
                delete[] prof;
                prof = bigger;
                prof_cap = S.prof_used;
            }
            if (S.map_used > map_cap) {
                uint16_t *bigger = msa_block<uint16_t>(S.map_used);
                memcpy(bigger, maps, map_cap * sizeof(uint16_t));
                delete[] maps;
                maps = bigger;
                map_cap = S.map_used;
            }
            uint32_t *tb = msa_block<uint32_t>(L.tb_words);
            uint8_t *ops = msa_block<uint8_t>(L.ops_bytes);
            uint64_t *row = msa_block<uint64_t>(L.row_entries);
            for (uint32_t x : msa_visit(L.count, order, rng))
                msa_host_merge(recs[x], X, G, prof, maps, tb, ops, row, lens, costs, order, rng, K);
            delete[] tb; delete[] ops; delete[] row;
            if (K) K->launches++;
        }
        for (const MsaLaunch &L : launches)
            if (status == SMX_OK) status = msa_launch_done(P, L, lens, &S, why);
    }
    if (status == SMX_OK) {
        out->n_cols = S.len[P.n_nodes - 1];
        memcpy(out->lens.data(), lens, P.n_merges * sizeof(uint32_t));
        memcpy(out->costs.data(), costs, P.n_merges * sizeof(uint64_t));
        if (out->n_cols > cap_cols) {
            *why = "overflow";
            status = SMX_ERR_OVERFLOW;
        } else {
            out->rows.assign((size_t)n * out->n_cols, 0x7b);
            msa_host_rows(bytes, doff.data(), n, P.parent.data(), S.map_off.data(), maps, out->n_cols, out->rows.data(), order, rng);
        }
    }
    delete[] prof; delete[] maps; delete[] lens; delete[] costs;
    return status;
}

}  // namespace smx

#endif  // MSA_HOST_H
