// smx_msa_core.h -- the arithmetic of the progressive alignment (smx_msa.hip), in integers and fixed to
// the last tie-break: the cost of a column pair, the three-way minimum with its direction code, the new column.  The
// kernels, the CPU simulation (tests/cpu/msa_host.h) and the sanitizer driver compile these functions and nothing else
// does the arithmetic, so a call's rows, lengths and costs are the same bytes on the device and on the host.
//
// A profile column holds six counts (A C G T other gap) whose sum is the number of tips under the node.  The five
// products of counts fit 32 bits (n_a n_b <= 4096^2 / 4); the weighted sums do not, so every score is 64 bits.
#ifndef SMX_MSA_CORE_H
#define SMX_MSA_CORE_H
#include <stdint.h>

#include "smx_hd.h"
#include "smx.h"   // SMX_MSA_MAX_N, SMX_MSA_MAX_COLS, smx_msa_merge

namespace smx {

// the shapes of the three kernels
constexpr unsigned MSA_TIPS_THREADS = 256;     // msa_tips_kernel: a thread per base
constexpr unsigned MSA_MERGE_THREADS = 1024;   // msa_merge_kernel: one workgroup per merge ...
constexpr unsigned MSA_WAVES = MSA_MERGE_THREADS / 64;   // ... its waves take consecutive bands of 64 rows
constexpr unsigned MSA_LAG = 2;                // blocks of 64 steps a wave stays behind the wave above it
constexpr unsigned MSA_ROWS_THREADS = 256;     // msa_rows_kernel: a workgroup per tip
constexpr unsigned MSA_TILE_ROWS = 64, MSA_TILE_WORDS = 16;   // the walk's LDS tile of direction words: 64 rows x 256 columns

constexpr uint32_t MSA_DIAG = 0, MSA_UP = 1, MSA_LEFT = 2;    // direction codes, two bits per cell, 16 cells per word
constexpr uint32_t MSA_NONE = 0xffffffffu;     // parent of the root
constexpr uint32_t MSA_GAP = 5;                // the gap's slot in a column

struct alignas(16) MsaCol { uint16_t c[8]; };  // six counts, c[6] = c[7] = 0: one 16-byte load

// One merge of a launch as the kernel sees it.  Offsets, not pointers: the profile and map buffers may move when they grow
struct MsaMergeDev {
    uint32_t t, La, Lb, na, nb, pad;           // the merge's index in the call; the children's lengths and tip counts
    uint64_t prof_a, prof_b, prof_out;         // columns into the profile buffer; prof_out has room for La + Lb
    uint64_t map_a, map_b;                     // entries into the map buffer: La and Lb of them
    uint64_t tb, ops, row;                     // the launch's scratch: La * msa_tb_words(Lb) words, La + Lb bytes, Lb + 1 scores
};

SMX_HD uint32_t msa_code(unsigned char ch) { return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u; }

SMX_HD MsaCol msa_tip_col(unsigned char ch) {
    const uint32_t code = msa_code(ch);
    MsaCol c = {{0, 0, 0, 0, 0, 0, 0, 0}};
    for (uint32_t s = 0; s < 5; s++) c.c[s] = (uint16_t)(code == s);
    return c;
}

SMX_HD uint32_t msa_tb_words(uint32_t Lb) { return (Lb + 15u) / 16u; }

// ga(i) = G ra n_b, gb(j) = G rb n_a: r = the column's residues, n_other = the tips of the other node
SMX_HD uint64_t msa_gap_cost(uint32_t G, uint32_t r, uint32_t n_other) { return (uint64_t)(G * r) * n_other; }

// s(i, j) = X (ra rb - sum_s ca[s] cb[s]) + G (ca[5] rb + ra cb[5])
SMX_HD uint64_t msa_pair_cost(const MsaCol &a, uint32_t ra, const MsaCol &b, uint32_t rb, uint32_t X, uint32_t G) {
    uint32_t same = 0;
    for (int s = 0; s < 5; s++) same += (uint32_t)a.c[s] * b.c[s];
    const uint32_t differ = ra * rb - same, gaps = (uint32_t)a.c[MSA_GAP] * rb + ra * (uint32_t)b.c[MSA_GAP];
    return (uint64_t)X * differ + (uint64_t)G * gaps;
}

// The three-way minimum and the direction the walk back takes from the cell: the diagonal if it reaches the minimum,
// else up, else left
SMX_HD uint64_t msa_min3(uint64_t diag, uint64_t up, uint64_t left, uint32_t *dir) {
    uint64_t best = diag < up ? diag : up;
    best = best < left ? best : left;
    *dir = best == diag ? MSA_DIAG : best == up ? MSA_UP : MSA_LEFT;
    return best;
}

// The new column of an op: both columns added, or one of them and the other node's tips as gaps
SMX_HD MsaCol msa_new_col(uint32_t op, const MsaCol &a, const MsaCol &b, uint32_t na, uint32_t nb) {
    MsaCol c = {{0, 0, 0, 0, 0, 0, 0, 0}};
    for (int s = 0; s < 6; s++) c.c[s] = (uint16_t)((op != MSA_LEFT ? a.c[s] : 0u) + (op != MSA_UP ? b.c[s] : 0u));
    if (op == MSA_UP) c.c[MSA_GAP] = (uint16_t)(c.c[MSA_GAP] + nb);
    if (op == MSA_LEFT) c.c[MSA_GAP] = (uint16_t)(c.c[MSA_GAP] + na);
    return c;
}

// the ops of thread x's chunk in the build phase: [lo, hi) of len ops
SMX_HD uint32_t msa_chunk(uint32_t len) { return (len + MSA_MERGE_THREADS - 1u) / MSA_MERGE_THREADS; }

}  // namespace smx

#endif  // SMX_MSA_CORE_H
