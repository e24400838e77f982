// smx_nj_core.h -- the arithmetic of the neighbour-joining call (smx_nj.hip), fixed to the last
// operation: every floating-point value the call records is the result of the IEEE double operations below, in the
// order written, each rounded on its own.  The kernels, the CPU simulation (tests/cpu/nj_host.h) and the sanitizer
// driver compile these functions and nothing else does the arithmetic, so the records are the same bits from run to
// run and from device to host.
//
// Contraction is off inside every function here (#pragma clang fp contract(off): hipcc contracts by default, and
// __dmul_rn / __dadd_rn are plain operators once inlined); the g++ builds of the tests pass -ffp-contract=off.
//
// The selection is a total order on (Q, lo, hi): any reduction order gives the same pair.  Finite inputs make NaN
// impossible, and a zero of either sign compares equal, so the order never looks at the sign of a zero.
#ifndef SMX_NJ_CORE_H
#define SMX_NJ_CORE_H
#include <stdint.h>

#include "smx_hd.h"
#include "smx.h"   // SMX_NJ_MAX_N, smx_nj_merge

#if defined(__clang__)
#define SMX_NJ_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SMX_NJ_NO_CONTRACT
#endif

namespace smx {

// the shapes of the three kernels; the plan (smx_nj_plan.h) sizes the grids by them
constexpr unsigned NJ_INIT_THREADS = 256;      // nj_init_kernel: a workgroup per row
constexpr unsigned NJ_ROWMIN_THREADS = 256;    // nj_rowmin_kernel: a wave per live row ...
constexpr unsigned NJ_ROWMIN_ROWS = NJ_ROWMIN_THREADS / 64;   // ... so this many rows per workgroup
constexpr unsigned NJ_JOIN_THREADS = 1024;     // nj_join_kernel: one workgroup, thread x owns the slots x, x + 1024, ...

// the workgroups of nj_rowmin_kernel at na live slots: the rows 0 .. na - 2 have a hi > lo
SMX_HD uint32_t nj_rowmin_grid(uint32_t na) { return (na - 1u + NJ_ROWMIN_ROWS - 1u) / NJ_ROWMIN_ROWS; }

// entry (i, j), i < j < n, of the packed upper triangle, row-major: the layout smx_pairs_distances writes
SMX_HD uint64_t nj_tri_index(uint32_t i, uint32_t j, uint32_t n) {
    return (uint64_t)i * n - (uint64_t)i * (i + 1u) / 2u + (j - i - 1u);
}

// step 1: Q of the slots lo < hi, c = double(na - 2): three operations, the smaller slot's r first
SMX_HD double nj_q(double c, double d, double r_lo, double r_hi) {
    SMX_NJ_NO_CONTRACT
    const double cd = c * d;
    const double t = cd - r_lo;
    return t - r_hi;
}

// step 2: is (q, lo, hi) before (q2, lo2, hi2)?
SMX_HD bool nj_before(double q, uint32_t lo, uint32_t hi, double q2, uint32_t lo2, uint32_t hi2) {
    if (q < q2) return true;
    if (q2 < q) return false;
    return lo != lo2 ? lo < lo2 : hi < hi2;
}

// step 4: the distance of slot k to the new node, dl = d[lo][hi]
SMX_HD double nj_duk(double d_lo_k, double d_hi_k, double dl) {
    SMX_NJ_NO_CONTRACT
    const double s = d_lo_k + d_hi_k;
    const double t = s - dl;
    return 0.5 * t;
}

// step 4: r[k] once the rows lo and hi have left the sum and the new node has joined it
SMX_HD double nj_r_other(double r_k, double d_lo_k, double d_hi_k, double duk) {
    SMX_NJ_NO_CONTRACT
    const double a = r_k - d_lo_k;
    const double b = a - d_hi_k;
    return b + duk;
}

// step 5: the new node's row sum in closed form, na = the active count before the merge
SMX_HD double nj_r_new(double ra, double rb, double na, double dl) {
    SMX_NJ_NO_CONTRACT
    const double s = ra + rb;
    const double p = na * dl;
    const double t = s - p;
    return 0.5 * t;
}

}  // namespace smx

#endif  // SMX_NJ_CORE_H
