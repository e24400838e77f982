// smx_chunk_plan.h -- what the host side of every chunked long-read call shares (specimine, clusters, consensus,
// crosstalk, identify): the state class of a pattern, the LDS bytes of its Peq table, the grid of a
// class's chunk list, the scratch of the generic class, the per-class launch table of a call (ChunkLaunches) with the
// walk over its launches, the pattern classes of a sequence list and its padded copy.  The bimera call
// (smx_reach_plan.h) takes the grid and the padded copy from here and has no classes.
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

// The launch table of a call: per state class its records (whatever the call's kernel walks: (job, query) pairs, rows,
// runs, jobs), their chunk prefix and the launch that takes them.  The plan of a call is one (MinePlan, PairsPlan,
// ConsPlan, NearestPlan and HitsPlan derive from it): it notes every pattern it will launch, appends its records class
// after class, and seals the table once.
struct ChunkLaunches {
    uint32_t n[CHUNK_CLASSES] = {0, 0, 0, 0, 0, 0};              // records per class
    std::vector<uint64_t> chunk_start;                           // per class with records: their chunk prefix, n + 1 entries
    uint64_t chunks[CHUNK_CLASSES] = {0, 0, 0, 0, 0, 0};
    uint64_t grid[CHUNK_CLASSES] = {0, 0, 0, 0, 0, 0};           // 0 for a class without records: nothing reads its per_block
    uint64_t per_block[CHUNK_CLASSES] = {1, 1, 1, 1, 1, 1};
    size_t lds_max[CHUNK_CLASSES] = {0, 0, 0, 0, 0, 0};          // the LDS bytes of the class's launch: its largest table
    int words_max0 = 0;                    // the generic class's longest pattern, in words
    uint64_t scratch_words = 0;            // u64 words of the generic class's state: grid[0] slices of 3 x words_max0 x lanes

    // a pattern of class c that will be launched: the LDS bytes of its table (0: not known, a lengths-only plan) and its words
    void note(int c, size_t lds, size_t W) {
        lds_max[c] = std::max(lds_max[c], lds);
        if (c == 0) words_max0 = std::max(words_max0, (int)W);
    }
    // a record of n_chunks chunks behind the records of class c; the classes are filled in ascending order
    void append(int c, uint64_t n_chunks) {
        if (!n[c]) chunk_start.push_back(0);
        n[c]++;
        chunks[c] += n_chunks;
        chunk_start.push_back(chunks[c]);
    }
    // The grids: `floor` chunks per workgroup, more only where the grid is capped: by grid_cap and the launch, and in
    // the generic class by the scratch slices of the workgroups in flight, which fit scratch_budget.
    void seal(uint64_t floor, uint64_t scratch_budget = CHUNK_SCRATCH_BYTES, uint64_t grid_cap = CHUNK_GRID_MAX) {
        for (int c = 0; c < CHUNK_CLASSES; c++) {
            if (!n[c]) continue;
            const uint64_t cap = c ? grid_cap : std::min(grid_cap, chunk_scratch_cap(words_max0, scratch_budget));
            const ChunkGrid G = chunk_grid(chunks[c], floor, cap);
            per_block[c] = G.per_block;
            grid[c] = G.grid;
        }
        scratch_words = chunk_scratch_words(grid[0], words_max0);
    }
    // forget the records and their grids and keep the noted patterns: a plan that is given its records more than once
    void clear_records() {
        chunk_start.clear();
        for (int c = 0; c < CHUNK_CLASSES; c++) { n[c] = 0; chunks[c] = 0; grid[c] = 0; per_block[c] = 1; }
        scratch_words = 0;
    }
    uint64_t grid_max() const { return *std::max_element(grid, grid + CHUNK_CLASSES); }
};

// The pattern classes of a sequence list (specimine's queries; clusters' reads, which may be empty): per sequence the LDS
// bytes of its Peq table and its state class.  Returns SMX_OK, or the status to fail with and why.
inline int chunk_pattern_classes(const char *queries, const uint64_t *qoff, uint32_t n_queries, bool allow_empty,
                                 std::vector<size_t> *qlds_out, std::vector<int> *qclass_out, std::string *why) {
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

// The padded copy of a sequence list (reads, refs, drafts, databases alike), as the kernels read it: 16-byte aligned
// copies, 16 bytes of slack at the end (a lane loads 16 bytes at a time).  Returns SMX_OK, or the status to fail with
// and why.
inline int chunk_padded_sequences(const char *seqs, const uint64_t *off, uint32_t n_seqs, std::vector<uint64_t> *doff_out,
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
// prefixes of n + 1 entries each.  launch(ChunkLaunch) runs for every class with records; the walk ends at the first
// nonzero return, which it returns.
struct ChunkLaunch {
    int c, wr;                 // the class and the wr of its launch
    uint32_t n;                // its records,
    size_t rec_at, start_at;   // where they and their chunk prefix begin in the call's lists
    int grid;
    uint64_t per_block;
    size_t lds;
};

template <typename F> inline int chunk_for_each_class(const ChunkLaunches &L, F &&launch) {
    size_t rec_at = 0, start_at = 0;
    for (int c = 0; c < CHUNK_CLASSES; c++) {
        if (!L.n[c]) continue;
        const ChunkLaunch K{c, CHUNK_CLASS_WORDS[c], L.n[c], rec_at, start_at, (int)L.grid[c], L.per_block[c], L.lds_max[c]};
        if (const int e = launch(K)) return e;
        rec_at += L.n[c];
        start_at += (size_t)L.n[c] + 1;
    }
    return 0;
}

}  // namespace smx

#endif  // SMX_CHUNK_PLAN_H
