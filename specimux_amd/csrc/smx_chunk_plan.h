// smx_chunk_plan.h -- what the host side of every chunked long-read call shares (specimine, clusters, consensus,
// crosstalk, identify): the state class of a pattern, the LDS bytes of its Peq table, the grid of a
// class's chunk list, the scratch of the generic class, the padded copy of the sequences and the walk over the classes
// of a call.  The bimera call (smx_reach_plan.h) takes the grid and the padded copy from here and has no classes.
// Host only and free of HIP calls, like the plans that use it (smx_cons_plan.h, smx_nearest_plan.h,
// smx_hits_plan.h, smx_reach_plan.h), so that the CPU simulations and the sanitizer drivers compile it as it is.
#ifndef SMX_CHUNK_PLAN_H
#define SMX_CHUNK_PLAN_H
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "smx_internal.h"

namespace smx {

// The state classes of a call: class 0 keeps a lane's state in global scratch (any length), classes 1..5 in registers.
constexpr int CHUNK_CLASSES = 6;
constexpr int CHUNK_CLASS_WORDS[CHUNK_CLASSES] = {0, 1, 2, 4, 8, 16};   // the wr of the class's launches
inline int chunk_class(size_t W) { return W <= 1 ? 1 : W <= 2 ? 2 : W <= 4 ? 3 : W <= 8 ? 4 : W <= 16 ? 5 : 0; }

constexpr uint64_t CHUNK_GRID_MAX = (uint64_t)INT32_MAX;          // workgroups of one launch
constexpr uint64_t CHUNK_SCRATCH_BYTES = (uint64_t)256 << 20;     // the generic class's per-lane state, at most (about)

// The Peq table of one pattern as mine_build_peq lays it out in LDS: the head, then (distinct bytes + 1) rows of W | 1 words.
struct ChunkTable {
    size_t W = 0, lds = 0;     // words of the pattern, LDS bytes of head and table
    int rows = 0, cls = 0;     // distinct bytes, state class
    bool fits() const { return lds <= SMX_LDS_POOL; }
    // why a call with this pattern is refused; who = "query 7: ", "job 3: the draft's ", ...
    std::string refusal(const std::string &who) const {
        return who + std::to_string(rows) + " distinct bytes x " + std::to_string(W) + " words do not fit the LDS (" +
               std::to_string(lds) + " > " + std::to_string((size_t)SMX_LDS_POOL) + " bytes)";
    }
};

inline ChunkTable chunk_table(const char *seq, uint64_t m) {
    ChunkTable T;
    bool seen[256] = {false};
    for (uint64_t i = 0; i < m; i++) {
        const unsigned char c = (unsigned char)seq[i];
        if (!seen[c]) { seen[c] = true; T.rows++; }
    }
    T.W = (size_t)((m + 63) / 64);
    T.lds = (MINE_LDS_HEAD + (size_t)(T.rows + 1) * (T.W | 1)) * 8;
    T.cls = chunk_class(T.W);
    return T;
}

// The grid of a class's chunks: workgroup b takes chunks [b * per_block, (b + 1) * per_block), at least `floor` of them
// (the call's own figure: what a workgroup should amortise its record search and table build over), more only where
// that would take more than `cap` workgroups.
struct ChunkGrid { uint64_t per_block = 1, grid = 0; };

inline ChunkGrid chunk_grid(uint64_t chunks, uint64_t floor, uint64_t cap) {
    cap = std::min(cap, CHUNK_GRID_MAX);
    ChunkGrid G;
    G.per_block = std::max(floor, (chunks + cap - 1) / cap);
    G.grid = (chunks + G.per_block - 1) / G.per_block;
    return G;
}

// The generic class keeps a lane's state in a global slice per workgroup (mine_lane_state, smx_mine_core.h):
// words_max0 = the class's longest pattern in words.  Its grid is capped so that the slices fit CHUNK_SCRATCH_BYTES,
// and the scratch is grid[0] slices: the kernels index it by blockIdx.x.
inline uint64_t chunk_slice_words(int words_max0) { return (uint64_t)3 * words_max0 * MINE_THREADS; }
// `budget` is CHUNK_SCRATCH_BYTES in production; a test passes less to cap the grid without gigabytes (one slice always goes).
inline uint64_t chunk_scratch_cap(int words_max0, uint64_t budget = CHUNK_SCRATCH_BYTES) {
    return std::max<uint64_t>(1, budget / std::max<uint64_t>(chunk_slice_words(words_max0) * 8, 1));
}
inline uint64_t chunk_scratch_words(uint64_t grid0, int words_max0) { return grid0 * chunk_slice_words(words_max0); }

// The grid of class c of a call: chunk_grid, the generic class's capped by its scratch as well.
inline ChunkGrid chunk_class_grid(int c, uint64_t chunks, uint64_t floor, int words_max0, uint64_t budget = CHUNK_SCRATCH_BYTES) {
    return chunk_grid(chunks, floor, c == 0 ? chunk_scratch_cap(words_max0, budget) : CHUNK_GRID_MAX);
}

// Per query (specimine) or read (clusters, which allows empty ones): the LDS bytes of its Peq table and its state class.
// Returns SMX_OK, or the status to fail with and why.
inline int mine_queries(const char *queries, const uint64_t *qoff, uint32_t n_queries, bool allow_empty, std::vector<size_t> *qlds_out,
                        std::vector<int> *qclass_out, std::string *why) {
    std::vector<size_t> &qlds = *qlds_out;
    std::vector<int> &qclass = *qclass_out;
    qlds.assign(n_queries, 0);
    qclass.assign(n_queries, 0);
    for (uint32_t q = 0; q < n_queries; q++) {
        if (qoff[q + 1] < qoff[q] || (qoff[q + 1] == qoff[q] && !allow_empty)) {
            *why = "query " + std::to_string(q) + " is empty";
            return SMX_ERR_ARG;
        }
        const uint64_t m = qoff[q + 1] - qoff[q];
        if (m > (uint64_t)INT32_MAX) {
            *why = "query " + std::to_string(q) + ": length " + std::to_string(m);
            return SMX_ERR_UNSUPPORTED;
        }
        const ChunkTable T = chunk_table(queries + qoff[q], m);
        if (!T.fits()) {
            *why = T.refusal("query " + std::to_string(q) + ": ");
            return SMX_ERR_UNSUPPORTED;
        }
        qlds[q] = T.lds;
        qclass[q] = T.cls;
    }
    return SMX_OK;
}

// The sequences as the kernels read them: 16-byte aligned copies, 16 bytes of slack at the end (a lane loads 16 bytes at
// a time).  Returns SMX_OK, or the status to fail with and why.
inline int mine_targets(const char *seqs, const uint64_t *off, uint32_t n_seqs, std::vector<uint64_t> *doff_out,
                        std::vector<int32_t> *len_out, std::vector<unsigned char> *pad, std::string *why) {
    std::vector<uint64_t> &doff = *doff_out;
    std::vector<int32_t> &len = *len_out;
    doff.assign(n_seqs, 0);
    len.assign(n_seqs, 0);
    uint64_t bytes = 0;
    for (uint32_t t = 0; t < n_seqs; t++) {
        if (off[t + 1] < off[t] || off[t + 1] - off[t] > (uint64_t)INT32_MAX) {
            *why = "target " + std::to_string(t) + ": bad offsets";
            return SMX_ERR_ARG;
        }
        doff[t] = bytes;
        len[t] = (int32_t)(off[t + 1] - off[t]);
        bytes += ((uint64_t)len[t] + 15) & ~(uint64_t)15;
    }
    bytes += 16;
    pad->assign(bytes, 0);
    for (uint32_t t = 0; t < n_seqs; t++) memcpy(pad->data() + doff[t], seqs + off[t], (size_t)len[t]);
    return SMX_OK;
}

// The launches of a call, class after class: the records of the classes lie one after the other, and so do their chunk
// prefixes of n + 1 entries each.  launch(class, wr, n, record offset, chunk_start offset) runs for every class with
// records; the walk ends at the first nonzero return, which it returns.
template <typename F> inline int chunk_for_each_class(const uint32_t (&n)[CHUNK_CLASSES], F &&launch) {
    size_t rat = 0, cat = 0;
    for (int c = 0; c < CHUNK_CLASSES; c++) {
        if (!n[c]) continue;
        if (const int e = launch(c, CHUNK_CLASS_WORDS[c], n[c], rat, cat)) return e;
        rat += n[c];
        cat += (size_t)n[c] + 1;
    }
    return 0;
}

}  // namespace smx

#endif  // SMX_CHUNK_PLAN_H
