// smx_msa_plan.h -- the host-side plan of one smx_msa call (smx_calls.cpp): the argument checks, the levels of the guide
// tree, the sizes of the device buffers, the cutting of a level into launches and the merge records a launch is handed
// (DESIGN.md §23).  Host only and free of HIP calls, so that the CPU simulation (tests/cpu/msa_sim.cpp) and the sanitizer
// driver (tests/asan/msa_driver.cpp) run it as it is.
//
// A child's length is known only once its level has run: msa_plan fixes what the arguments alone decide (levels,
// parents, tip counts), and MsaState carries what the call learns level by level (lengths, offsets).
#ifndef SMX_MSA_PLAN_H
#define SMX_MSA_PLAN_H
#include <string>
#include <vector>

#include "smx_msa_core.h"

namespace smx {

// what one launch may keep in scratch (direction words, ops, hand-over rows) unless the caller's environment says
// otherwise (SMX_CLUSTERS_BUDGET_BYTES, else SMX_MINE_BUDGET_BYTES, as clusters.budget_bytes() reads them); one merge
// always goes
constexpr uint64_t MSA_DEFAULT_BUDGET = 1ull << 30;

struct MsaPlan {
    uint32_t n = 0, n_merges = 0, n_nodes = 0, n_levels = 0;   // n_levels: the root's level (0 for n <= 1)
    uint64_t seq_bytes = 0;
    std::vector<uint32_t> level, parent, tips;   // per node: its level, its parent (MSA_NONE: the root), the tips under it
    std::vector<uint32_t> order;                 // the merges level by level, in index order within a level
    std::vector<uint32_t> level_start;           // n_levels + 1 entries into order: level v + 1's merges are [v], [v + 1])
};

// The plan of a call.  Returns SMX_OK, or the status to fail with and why.
inline int msa_plan(const char *seqs, const uint64_t *off, uint32_t n, const smx_msa_merge *merges, uint32_t X, uint32_t G,
                    const uint8_t *rows, const uint32_t *n_cols, const uint32_t *lens, const uint64_t *costs, MsaPlan *plan,
                    std::string *why) {
    MsaPlan &P = *plan;
    P = MsaPlan();
    if (!n_cols || (n >= 1 && (!seqs || !off || !rows)) || (n >= 2 && (!merges || !lens || !costs))) {
        *why = "null argument";
        return SMX_ERR_ARG;
    }
    if (X < 1 || X > 1000 || G < 1 || G > 1000) {
        *why = "weights " + std::to_string(X) + ", " + std::to_string(G) + " outside 1..1000";
        return SMX_ERR_ARG;
    }
    if (n > (uint32_t)SMX_MSA_MAX_N) {
        *why = "n = " + std::to_string(n) + " above " + std::to_string(SMX_MSA_MAX_N) + " sequences";
        return SMX_ERR_UNSUPPORTED;
    }
    for (uint32_t i = 0; i < n; i++) {
        if (off[i + 1] <= off[i]) {
            *why = "sequence " + std::to_string(i) + " is empty";
            return SMX_ERR_ARG;
        }
        if (off[i + 1] - off[i] > (uint64_t)SMX_MSA_MAX_COLS) {
            *why = "sequence " + std::to_string(i) + " is longer than " + std::to_string(SMX_MSA_MAX_COLS);
            return SMX_ERR_UNSUPPORTED;
        }
    }
    P.n = n;
    P.n_merges = n ? n - 1 : 0;
    P.n_nodes = n + P.n_merges;
    P.seq_bytes = n ? off[n] - off[0] : 0;
    P.level.assign(P.n_nodes, 0);
    P.parent.assign(P.n_nodes, MSA_NONE);
    P.tips.assign(P.n_nodes, 1);
    for (uint32_t t = 0; t < P.n_merges; t++) {
        const uint32_t a = merges[t].a, b = merges[t].b, node = n + t;
        if (a == b || a >= node || b >= node || P.parent[a] != MSA_NONE || P.parent[b] != MSA_NONE) {
            *why = "merge " + std::to_string(t) + " (" + std::to_string(a) + ", " + std::to_string(b) + ") is not one of the tree";
            return SMX_ERR_ARG;
        }
        P.parent[a] = P.parent[b] = node;
        P.tips[node] = P.tips[a] + P.tips[b];
        P.level[node] = 1 + (P.level[a] > P.level[b] ? P.level[a] : P.level[b]);
    }
    P.n_levels = P.n_merges ? P.level[P.n_nodes - 1] : 0;
    // n - 1 merges, every node a child at most once and every child older than its parent: the last node is the root
    std::vector<uint32_t> count(P.n_levels + 1, 0);
    for (uint32_t t = 0; t < P.n_merges; t++) count[P.level[n + t]]++;
    P.level_start.assign(P.n_levels + 1, 0);
    for (uint32_t v = 1; v <= P.n_levels; v++) P.level_start[v] = P.level_start[v - 1] + count[v];
    P.order.assign(P.n_merges, 0);
    std::vector<uint32_t> at(P.level_start.begin(), P.level_start.end());
    for (uint32_t t = 0; t < P.n_merges; t++) P.order[at[P.level[n + t] - 1]++] = t;
    return SMX_OK;
}

// What the call knows of the nodes so far: the lengths of the nodes whose level has run, and where their profiles and
// maps are.  Profile offsets count columns (16 bytes), map offsets entries (2 bytes).
struct MsaState {
    std::vector<uint32_t> len;                   // per node, 0 until known
    std::vector<uint64_t> prof_off, map_off;     // per node; map_off of a node is set when it becomes a child
    uint64_t prof_used = 0, map_used = 0;        // the columns and entries handed out
};

// the tips' profiles, one after the other
inline void msa_state_init(const MsaPlan &P, const uint64_t *off, MsaState *S) {
    S->len.assign(P.n_nodes, 0);
    S->prof_off.assign(P.n_nodes, 0);
    S->map_off.assign(P.n_nodes, 0);
    S->prof_used = S->map_used = 0;
    for (uint32_t i = 0; i < P.n; i++) {
        S->len[i] = (uint32_t)(off[i + 1] - off[i]);
        S->prof_off[i] = S->prof_used;
        S->prof_used += S->len[i];
    }
}

struct MsaLaunch {
    uint32_t first = 0, count = 0;               // P.order[first .. first + count)
    uint64_t tb_words = 0, ops_bytes = 0, row_entries = 0;   // the launch's scratch
    uint64_t bytes() const { return tb_words * 4 + ops_bytes + row_entries * 8; }
};

inline void msa_merge_scratch(uint32_t La, uint32_t Lb, uint64_t *tb_words, uint64_t *ops_bytes, uint64_t *row_entries) {
    *tb_words = (uint64_t)La * msa_tb_words(Lb);
    *ops_bytes = (uint64_t)La + Lb;
    *row_entries = (uint64_t)Lb + 1;
}

// Level v (1 .. n_levels) cut into launches of at most `budget` scratch bytes each; a merge that alone exceeds the
// budget gets a launch of its own.  The children's lengths are known.
inline void msa_level_launches(const MsaPlan &P, const smx_msa_merge *merges, const MsaState &S, uint32_t v, uint64_t budget,
                               std::vector<MsaLaunch> *out) {
    out->clear();
    MsaLaunch cur;
    cur.first = P.level_start[v - 1];
    for (uint32_t x = P.level_start[v - 1]; x < P.level_start[v]; x++) {
        const smx_msa_merge &m = merges[P.order[x]];
        MsaLaunch one;
        msa_merge_scratch(S.len[m.a], S.len[m.b], &one.tb_words, &one.ops_bytes, &one.row_entries);
        if (cur.count && cur.bytes() + one.bytes() > budget) {
            out->push_back(cur);
            cur = MsaLaunch();
            cur.first = x;
        }
        cur.count++;
        cur.tb_words += one.tb_words;
        cur.ops_bytes += one.ops_bytes;
        cur.row_entries += one.row_entries;
    }
    if (cur.count) out->push_back(cur);
}

// The records of a launch, and the room its new nodes and its children's maps take: prof_used and map_used grow
inline void msa_launch_records(const MsaPlan &P, const smx_msa_merge *merges, const MsaLaunch &L, MsaState *S,
                               std::vector<MsaMergeDev> *recs) {
    recs->assign(L.count, MsaMergeDev());
    uint64_t tb = 0, ops = 0, row = 0;
    for (uint32_t x = 0; x < L.count; x++) {
        const uint32_t t = P.order[L.first + x], a = merges[t].a, b = merges[t].b, node = P.n + t;
        MsaMergeDev &R = (*recs)[x];
        R.t = t; R.La = S->len[a]; R.Lb = S->len[b]; R.na = P.tips[a]; R.nb = P.tips[b]; R.pad = 0;
        R.prof_a = S->prof_off[a]; R.prof_b = S->prof_off[b];
        R.prof_out = S->prof_off[node] = S->prof_used;
        S->prof_used += (uint64_t)R.La + R.Lb;
        R.map_a = S->map_off[a] = S->map_used;
        R.map_b = S->map_off[b] = S->map_used + R.La;
        S->map_used += (uint64_t)R.La + R.Lb;
        R.tb = tb; R.ops = ops; R.row = row;
        uint64_t w, o, r;
        msa_merge_scratch(R.La, R.Lb, &w, &o, &r);
        tb += w; ops += o; row += r;
    }
}

// After a launch: the new nodes' lengths from lens.  Returns SMX_ERR_UNSUPPORTED for a node above SMX_MSA_MAX_COLS.
inline int msa_launch_done(const MsaPlan &P, const MsaLaunch &L, const uint32_t *lens, MsaState *S, std::string *why) {
    for (uint32_t x = 0; x < L.count; x++) {
        const uint32_t t = P.order[L.first + x];
        S->len[P.n + t] = lens[t];
        if (lens[t] > (uint32_t)SMX_MSA_MAX_COLS) {
            *why = "node " + std::to_string(P.n + t) + " has " + std::to_string(lens[t]) + " columns, above " +
                   std::to_string(SMX_MSA_MAX_COLS);
            return SMX_ERR_UNSUPPORTED;
        }
    }
    return SMX_OK;
}

}  // namespace smx

#endif  // SMX_MSA_PLAN_H
