// smx_nj_plan.h -- the host-side plan of one smx_nj call (smx_calls.cpp): the argument checks, the sizes of the device
// buffers, the launch counts and the grids, and the answer of a call too small to launch anything.
// Host only and free of HIP calls, so that the CPU simulation (tests/cpu/nj_sim.cpp) and the sanitizer driver
// (tests/asan/nj_driver.cpp) run it as it is.
#ifndef SMX_NJ_PLAN_H
#define SMX_NJ_PLAN_H
#include <string>

#include "smx_nj_core.h"

namespace smx {

struct NjPlan {
    uint32_t n = 0;
    uint32_t iterations = 0;          // max(n - 3, 0): merge t runs with n - t live slots
    uint64_t launches = 0;            // one init launch and two per iteration; 0 for n <= 3
    uint64_t tri_entries = 0;         // n (n - 1) / 2
    // device buffers, in bytes
    uint64_t tri_bytes = 0;           // the caller's triangle
    uint64_t d_bytes = 0;             // n x n doubles, row stride n
    uint64_t r_bytes = 0;             // n doubles
    uint64_t node_bytes = 0;          // n uint32
    uint64_t best_q_bytes = 0;        // per row its smallest Q: n doubles (rows 0 .. na - 2 are written and read)
    uint64_t best_hi_bytes = 0;       // and the hi it belongs to: n uint32
    uint64_t merges_bytes = 0;        // iterations records
    uint32_t init_grid = 0;           // a workgroup per row
    uint32_t rowmin_grid_max = 0;     // the first iteration's: nj_rowmin_grid(n)
};

// The plan of a call.  Returns SMX_OK, or the status to fail with and why.
inline int nj_plan(const int32_t *tri, uint32_t n, const smx_nj_merge *merges, const uint32_t *last, const double *last_d,
                   NjPlan *plan, std::string *why) {
    NjPlan &P = *plan;
    P = NjPlan();
    if (!last || !last_d || (n >= 2 && !tri) || (n > 3 && !merges)) {
        *why = "null argument";
        return SMX_ERR_ARG;
    }
    if (n > (uint32_t)SMX_NJ_MAX_N) {
        *why = "n = " + std::to_string(n) + " above " + std::to_string(SMX_NJ_MAX_N) + " tips";
        return SMX_ERR_UNSUPPORTED;
    }
    P.n = n;
    P.tri_entries = (uint64_t)n * (n ? n - 1u : 0u) / 2u;
    for (uint64_t x = 0; x < P.tri_entries; x++)
        if (tri[x] < 0) {
            *why = "distance " + std::to_string(x) + " is negative";
            return SMX_ERR_ARG;
        }
    P.iterations = n > 3 ? n - 3 : 0;
    if (P.iterations == 0) return SMX_OK;
    P.launches = 1 + 2 * (uint64_t)P.iterations;
    P.tri_bytes = P.tri_entries * sizeof(int32_t);
    P.d_bytes = (uint64_t)n * n * sizeof(double);
    P.r_bytes = P.best_q_bytes = (uint64_t)n * sizeof(double);
    P.node_bytes = P.best_hi_bytes = (uint64_t)n * sizeof(uint32_t);
    P.merges_bytes = (uint64_t)P.iterations * sizeof(smx_nj_merge);
    P.init_grid = n;
    P.rowmin_grid_max = nj_rowmin_grid(n);
    return SMX_OK;
}

// The answer of a call with n <= 3: the nodes 0 .. n - 1 and the given distances, the rest zeroed.
inline void nj_small(const int32_t *tri, uint32_t n, uint32_t last[3], double last_d[3]) {
    for (uint32_t i = 0; i < 3; i++) {
        last[i] = i < n ? i : 0u;
        last_d[i] = 0.0;
    }
    if (n == 2) last_d[0] = (double)tri[0];
    if (n == 3)
        for (uint32_t i = 0; i < 3; i++) last_d[i] = (double)tri[i];   // (0, 1), (0, 2), (1, 2): the triangle's own order
}

}  // namespace smx

#endif  // SMX_NJ_PLAN_H
