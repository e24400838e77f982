// nj_host.h -- the three kernels of smx_nj.hip as host loops over smx_nj_core.h, thread for thread: the same index
// expressions, the same per-lane and per-thread partial results, the same phases.  Where the kernel reduces over lanes,
// waves or threads, or lets the threads of a phase run in any order, the loops here visit them in the order the caller
// asks for (forward, reversed, shuffled): the records may not depend on it.  Shared by tests/cpu/nj_sim.cpp and
// tests/asan/nj_driver.cpp; the buffers are the caller's, of the sizes smx_nj_plan.h gives.
#ifndef NJ_HOST_H
#define NJ_HOST_H
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "smx_nj_plan.h"

namespace smx {

enum NjOrder { NJ_FORWARD = 0, NJ_REVERSED = 1, NJ_SHUFFLED = 2 };

struct NjCounters {
    uint64_t iterations = 0, ties = 0, moves_none = 0, moves = 0, rowmin_rows = 0, rowmin_entries = 0, join_slots = 0;
};

struct NjCand { double q; uint32_t lo, hi; };
constexpr uint32_t NJ_HOST_NONE = 0xffffffffu;

// the indices 0 .. count - 1 in the order asked for
inline std::vector<uint32_t> nj_visit(uint32_t count, NjOrder order, std::mt19937 &rng) {
    std::vector<uint32_t> v(count);
    std::iota(v.begin(), v.end(), 0u);
    if (order == NJ_REVERSED) std::reverse(v.begin(), v.end());
    if (order == NJ_SHUFFLED) std::shuffle(v.begin(), v.end(), rng);
    return v;
}

// the smallest of the candidates, folded in the order asked for
inline NjCand nj_fold(const std::vector<NjCand> &c, NjOrder order, std::mt19937 &rng, NjCounters *K) {
    NjCand best{INFINITY, NJ_HOST_NONE, NJ_HOST_NONE};
    for (uint32_t x : nj_visit((uint32_t)c.size(), order, rng)) {
        if (K && c[x].q == best.q && c[x].lo != NJ_HOST_NONE) K->ties++;
        if (nj_before(c[x].q, c[x].lo, c[x].hi, best.q, best.lo, best.hi)) best = c[x];
    }
    return best;
}

// nj_init_kernel: workgroup i, thread x takes the columns x, x + NJ_INIT_THREADS, ...
inline void nj_host_init(const int32_t *tri, uint32_t n, double *d, double *r, uint32_t *node) {
    for (uint32_t i = 0; i < n; i++) {
        double *row = d + (size_t)i * n;
        long long total = 0;
        for (uint32_t x = 0; x < NJ_INIT_THREADS; x++) {
            long long sum = 0;
            for (uint32_t j = x; j < n; j += NJ_INIT_THREADS) {
                const int32_t v = j == i ? 0 : tri[i < j ? nj_tri_index(i, j, n) : nj_tri_index(j, i, n)];
                row[j] = (double)v;
                sum += v;
            }
            total += sum;
        }
        r[i] = (double)total;
        node[i] = i;
    }
}

// nj_rowmin_kernel at na live slots: the waves of a grid of nj_rowmin_grid(na) workgroups
inline void nj_host_rowmin(const double *d, const double *r, uint32_t n, uint32_t na, double *best_q, uint32_t *best_hi,
                           NjOrder order, std::mt19937 &rng, NjCounters *K) {
    const uint32_t grid = nj_rowmin_grid(na);
    for (uint32_t wave : nj_visit(grid * NJ_ROWMIN_ROWS, order, rng)) {
        const uint32_t lo = wave;               // blockIdx.x * NJ_ROWMIN_ROWS + the wave within the workgroup
        if (lo + 1u >= na) continue;
        const double c = (double)(na - 2u), r_lo = r[lo];
        const double *row = d + (size_t)lo * n;
        std::vector<NjCand> lanes(64, NjCand{INFINITY, lo, NJ_HOST_NONE});
        for (uint32_t lane = 0; lane < 64; lane++)
            for (uint32_t hi = lo + 1u + lane; hi < na; hi += 64u) {
                const double v = nj_q(c, row[hi], r_lo, r[hi]);
                if (nj_before(v, lo, hi, lanes[lane].q, lo, lanes[lane].hi)) lanes[lane] = NjCand{v, lo, hi};
                if (K) K->rowmin_entries++;
            }
        for (NjCand &l : lanes) if (l.hi == NJ_HOST_NONE) l.lo = NJ_HOST_NONE;    // an idle lane offers nothing
        const NjCand best = nj_fold(lanes, order, rng, nullptr);
        best_q[lo] = best.q;
        best_hi[lo] = best.hi;
        if (K) K->rowmin_rows++;
    }
}

// nj_join_kernel: merge t at na live slots.  Returns false if the pair is not one (the kernel returns early then).
inline bool nj_host_join(double *d, double *r, uint32_t *node, uint32_t n, uint32_t na, uint32_t t, const double *best_q,
                         const uint32_t *best_hi, smx_nj_merge *merges, NjOrder order, std::mt19937 &rng, NjCounters *K) {
    // A: every thread's own smallest, then the fold over the threads
    std::vector<NjCand> threads(NJ_JOIN_THREADS, NjCand{INFINITY, NJ_HOST_NONE, NJ_HOST_NONE});
    for (uint32_t tid = 0; tid < NJ_JOIN_THREADS; tid++)
        for (uint32_t row = tid; row + 1u < na; row += NJ_JOIN_THREADS)
            if (nj_before(best_q[row], row, best_hi[row], threads[tid].q, threads[tid].lo, threads[tid].hi))
                threads[tid] = NjCand{best_q[row], row, best_hi[row]};
    const NjCand pair = nj_fold(threads, order, rng, K);
    const uint32_t lo = pair.lo, hi = pair.hi;
    if (lo >= hi || hi >= na) return false;
    // B
    double *row_lo = d + (size_t)lo * n, *row_hi = d + (size_t)hi * n;
    const double dl = row_lo[hi], ra = r[lo], rb = r[hi];
    smx_nj_merge m;
    memset(&m, 0, sizeof m);
    m.a = node[lo]; m.b = node[hi]; m.n_active = na; m.pad = 0u;
    m.d = dl; m.ra = ra; m.rb = rb;
    merges[t] = m;
    // C: the threads in any order
    for (uint32_t tid : nj_visit(NJ_JOIN_THREADS, order, rng))
        for (uint32_t k = tid; k < na; k += NJ_JOIN_THREADS) {
            if (k == lo || k == hi) continue;
            const double a = row_lo[k], b = row_hi[k];
            const double duk = nj_duk(a, b, dl);
            r[k] = nj_r_other(r[k], a, b, duk);
            row_lo[k] = duk;
            d[(size_t)k * n + lo] = duk;
            if (K) K->join_slots++;
        }
    r[lo] = nj_r_new(ra, rb, (double)na, dl);
    node[lo] = n + t;
    // D
    const uint32_t last = na - 1u;
    if (hi != last) {
        const double *row_last = d + (size_t)last * n;
        for (uint32_t tid : nj_visit(NJ_JOIN_THREADS, order, rng))
            for (uint32_t k = tid; k < last; k += NJ_JOIN_THREADS) {
                if (k == hi) continue;
                const double v = row_last[k];
                row_hi[k] = v;
                d[(size_t)k * n + hi] = v;
            }
        row_hi[hi] = 0.0;
        r[hi] = r[last];
        node[hi] = node[last];
        if (K) K->moves++;
    } else if (K) {
        K->moves_none++;
    }
    if (K) K->iterations++;
    return true;
}

// What smx_nj computes, over buffers of exactly the planned sizes.  Returns the plan's status.
struct NjHostResult {
    std::vector<smx_nj_merge> merges;
    uint32_t last[3] = {0, 0, 0};
    double last_d[3] = {0, 0, 0};
};

inline int nj_host_call(const int32_t *tri, uint32_t n, NjOrder order, uint32_t seed, NjHostResult *out, NjCounters *K,
                        std::string *why) {
    NjPlan P;
    smx_nj_merge none = {};
    const int rc = nj_plan(tri, n, &none, out->last, out->last_d, &P, why);
    if (rc != SMX_OK) return rc;
    out->merges.assign(P.iterations, smx_nj_merge());
    if (P.iterations == 0) {
        nj_small(tri, n, out->last, out->last_d);
        return SMX_OK;
    }
    std::mt19937 rng(seed);
    // heap blocks of exactly the planned bytes: an index the plan did not budget for is a heap overflow under ASan
    double *d = new double[P.d_bytes / sizeof(double)], *r = new double[P.r_bytes / sizeof(double)];
    double *best_q = new double[P.best_q_bytes / sizeof(double)];
    uint32_t *node = new uint32_t[P.node_bytes / 4], *best_hi = new uint32_t[P.best_hi_bytes / 4];
    smx_nj_merge *merges = new smx_nj_merge[P.merges_bytes / sizeof(smx_nj_merge)];
    // what an earlier call may have left: never zero, never a live value
    memset(d, 0x7b, P.d_bytes); memset(r, 0x7b, P.r_bytes); memset(best_q, 0x7b, P.best_q_bytes);
    memset(node, 0x7b, P.node_bytes); memset(best_hi, 0x7b, P.best_hi_bytes);
    nj_host_init(tri, n, d, r, node);
    bool good = true;
    for (uint32_t t = 0; good && t + 3u < n; t++) {
        const uint32_t na = n - t;
        nj_host_rowmin(d, r, n, na, best_q, best_hi, order, rng, K);
        good = nj_host_join(d, r, node, n, na, t, best_q, best_hi, merges, order, rng, K);
    }
    if (good) {
        memcpy(out->merges.data(), merges, P.merges_bytes);
        for (int i = 0; i < 3; i++) out->last[i] = node[i];
        out->last_d[0] = d[1]; out->last_d[1] = d[2]; out->last_d[2] = d[(size_t)n + 2];
    }
    delete[] d; delete[] r; delete[] best_q; delete[] node; delete[] best_hi; delete[] merges;
    if (!good) { *why = "the join found no pair"; return SMX_ERR_ARG; }
    return SMX_OK;
}

}  // namespace smx

#endif  // NJ_HOST_H
