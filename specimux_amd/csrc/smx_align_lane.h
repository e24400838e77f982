// smx_align_lane.h -- one alignment of smx_align and of smx_align_batch as a function over pointers: what one lane of
// align_kernel / align_batch_kernel (smx_align.hip) does.  The kernels keep only the lane index and the call.  The CPU twin
// (tests/cpu/align_sim.cpp) and the sanitizer driver (tests/asan/align_driver.cpp) compile these same lines over heap
// buffers of the sizes smx_calls.cpp allocates; for them tests/cpu/align_host.h defines the device qualifiers away.
#ifndef SMX_ALIGN_LANE_H
#define SMX_ALIGN_LANE_H
#include "smx_align_core.h"

namespace smx {

// Columns of a target of n letters that an alignment scans.  HW: all of them; the score of a column never exceeds m <= 64.
// SHW: the one-letter prefix costs at most m, so best <= m, and the prefix of j letters costs at least j - m; an optimal
// end within k therefore lies in the first m + min(k, m) columns, and the minimum over those columns is the minimum over
// all whenever that is within k.  (k < 0: no column, the result is "above k" as for every k < best.)
__device__ __forceinline__ int align_scan_len(int m, int n, int k, int mode) {
    if (mode != 1) return n;
    const int lim = m + (k < 0 ? 0 : k < m ? k : m);
    return n < lim ? n : lim;
}

// edlib's start rule for an optimal end at column j: the last optimal position of the reversed problem, over at most
// m + best columns to the left
__device__ __forceinline__ int align_start_of(const unsigned long long *rpeq, int m, const unsigned char *t, int j, int best) {
    const int top = m - 1;
    unsigned long long P2 = ~0ull, M2 = 0;
    int sc = m, lastc = 1;
    for (int c = 1; c <= m + best && j - (c - 1) >= 0; c++) {
        myers_step<unsigned long long, true>(rpeq[t[j - (c - 1)]], P2, M2, sc, top);
        if (sc == best) lastc = c;
    }
    return j - (lastc - 1);
}

// smx_align: one target of n letters (codes 0..15); endflag and starts hold n entries each.  *out_dist = -1 leaves both
// unspecified; otherwise endflag[j] = 1 where column j is an optimal end, and starts[j] its start.
__device__ __forceinline__ void align_lane(const unsigned long long *peq, const unsigned long long *rpeq, int m,
                                           const unsigned char *tcodes, int n, int k, int mode, int *out_dist,
                                           unsigned char *endflag, int *starts) {
    const int nt = align_scan_len(m, n, k, mode), top = m - 1;
    unsigned long long Pv = ~0ull, Mv = 0;
    int score = m, best = m + 1;
    for (int j = 0; j < nt; j++) {
        if (mode == 0) myers_step<unsigned long long, false>(peq[tcodes[j]], Pv, Mv, score, top);
        else myers_step<unsigned long long, true>(peq[tcodes[j]], Pv, Mv, score, top);
        if (score < best) best = score;
        // raw score, thresholded below.  One byte holds it: HW scores are <= m <= 64, and an SHW score of the nt <= 2 m
        // columns scanned (align_scan_len) is at most max(m, j + 1) <= 128, so no two scores share a byte value
        endflag[j] = (unsigned char)score;
    }
    if (best > k) { *out_dist = -1; return; }
    *out_dist = best;
    for (int j = 0; j < n; j++) {
        const bool hit = j < nt && endflag[j] == (unsigned char)best;
        endflag[j] = hit ? 1 : 0;
        starts[j] = hit && mode == 0 ? align_start_of(rpeq, m, tcodes, j, best) : 0;
    }
}

// Host side of smx_align: what align_lane left, as locations.  The first min(count, cap) optimal ends and their starts go to
// starts / ends (which may be null: nothing is written); returns the count.
inline int align_collect(int dist, const unsigned char *endflag, const int *st, int n, int *starts, int *ends, int cap) {
    int cnt = 0;
    if (dist >= 0)
        for (int j = 0; j < n; j++)
            if (endflag[j]) {
                if (cnt < cap && starts && ends) { starts[cnt] = st[j]; ends[cnt] = j; }
                cnt++;
            }
    return cnt;
}

// smx_align_batch: alignment i of the launch.  q_peq: per distinct query 32 words (Peq of the query, then Peq of the
// reversed query); the raw scores of alignment i go to ws[toff[i] .. toff[i + 1]), its first min(nloc, cap) locations to
// out_starts / out_ends[i * cap ..), which are never touched where cap == 0.
__device__ __forceinline__ void align_batch_lane(unsigned i, const unsigned long long *q_peq, const int *q_len, const unsigned *qidx,
                                                 const unsigned char *tcodes, const unsigned long long *toff, const int *kk,
                                                 const unsigned char *modes, unsigned char *ws, int *out_dist, int *out_nloc,
                                                 int *out_starts, int *out_ends, unsigned cap) {
    const unsigned long long *peq = q_peq + (size_t)qidx[i] * 32, *rpeq = peq + 16;
    const int m = q_len[qidx[i]], k = kk[i], mode = modes[i], top = m - 1;
    const unsigned char *t = tcodes + toff[i];
    const int nt = align_scan_len(m, (int)(toff[i + 1] - toff[i]), k, mode);
    unsigned char *sc = ws + toff[i];
    unsigned long long Pv = ~0ull, Mv = 0;
    int score = m, best = m + 1;
    for (int j = 0; j < nt; j++) {
        if (mode == 0) myers_step<unsigned long long, false>(peq[t[j]], Pv, Mv, score, top);
        else myers_step<unsigned long long, true>(peq[t[j]], Pv, Mv, score, top);
        best = score < best ? score : best;
        sc[j] = (unsigned char)score;   // at most 128, as in align_lane: the byte cannot wrap
    }
    if (best > k) { out_dist[i] = -1; out_nloc[i] = 0; return; }
    out_dist[i] = best;
    int cnt = 0;
    for (int j = 0; j < nt; j++) {
        if (sc[j] != (unsigned char)best) continue;
        if ((unsigned)cnt < cap) {
            out_starts[(size_t)i * cap + cnt] = mode == 0 ? align_start_of(rpeq, m, t, j, best) : 0;
            out_ends[(size_t)i * cap + cnt] = j;
        }
        cnt++;
    }
    out_nloc[i] = cnt;
}

}  // namespace smx
#endif
