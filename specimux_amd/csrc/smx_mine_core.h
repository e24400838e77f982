// smx_mine_core.h -- the per-pair code of the specimine kernel (smx_mine.hip): HW (infix) edit distance of one query,
// given as a Peq table and a byte -> row map, in one target, by the multi-word Myers/Hyyro bit-vector with an
// edlib-style block band:
//   * blocks 0..L hold the column's state; a block is dropped from the bottom once its bottom score is >= k + 64
//     (every cell of it is then > k), and block L+1 joins a column only if the bottom cell of L was <= k one column
//     earlier (diagonals never decrease, so no cell deeper than that can reach <= k).  A block that joins starts
//     from the +1-per-row column, an upper bound of the true one; cells <= k are still exact.
//   * once a column's last-row score v <= k is found, k tightens to v (only the minimum is wanted).
//
// This header is host/device code: the kernel and the CPU unit test (tests/cpu/mine_sim.cpp) run the same functions;
// on the host the Peq table is a plain array and a "lane" is one call.  Device-only intrinsics sit behind the small
// wrappers below (popcount, min, the 16-byte target word).
#ifndef SMX_MINE_CORE_H
#define SMX_MINE_CORE_H
#include <stddef.h>
#include <stdint.h>
#include "smx_hd.h"

#if defined(__HIPCC__)
#define SMX_MINE_HD __host__ __device__
#else
#define SMX_MINE_HD
#endif

// one work item = one query x up to MINE_THREADS targets, one target per lane
#define MINE_THREADS 128

namespace smx {

typedef unsigned long long u64;

// 16 target bytes, one global_load_dwordx4 on the device.  A host caller keeps its targets in arrays of mine_u4.
#if defined(__HIPCC__)
typedef uint4 mine_u4;
SMX_HD mine_u4 mine_u4_zero() { return make_uint4(0, 0, 0, 0); }
#else
struct alignas(16) mine_u4 { unsigned x, y, z, w; };
SMX_HD mine_u4 mine_u4_zero() { return mine_u4{0, 0, 0, 0}; }
#endif

SMX_HD int mine_popc(u64 x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}

SMX_HD int mine_min(int a, int b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return min(a, b);
#else
    return a < b ? a : b;
#endif
}

// The arithmetic of the owner search of a chunk walk (chunk_owner, smx_mine_lds.h), which keeps the ballot: the record
// is in [p, p + n).  A round probes 64 records step = chunk_owner_step(n) apart, lane l the record
// chunk_owner_probe(p, step, l) if that is below p + n; "chunk_start[probe] <= lo" holds on a prefix of the lanes (lane
// 0 always), and with `count` lanes holding, the record is in the step-wide range of the last of them.  The host twin
// (tests/cpu/chunk_owner_host.h) runs the same functions over 64 emulated lanes.
SMX_HD uint32_t chunk_owner_step(uint32_t n) { return (n + 63) / 64; }
SMX_HD uint32_t chunk_owner_probe(uint32_t p, uint32_t step, unsigned lane) { return p + lane * step; }
// the range after the round: it starts chunk_owner_advance(step, count) records further on and holds
// chunk_owner_left(step, end, p) records, p the new start and end the old p + n
SMX_HD uint32_t chunk_owner_advance(uint32_t step, uint32_t count) { return (count - 1) * step; }
SMX_HD uint32_t chunk_owner_left(uint32_t step, uint32_t end, uint32_t p) { return step < end - p ? step : end - p; }

// Hyyro's block step with a horizontal carry in and out (hin, hout in {-1, 0, +1}).
SMX_HD int mine_step(u64 Eq, u64 &Pv, u64 &Mv, int hin) {
    const u64 hneg = hin < 0 ? 1ull : 0ull, hpos = hin > 0 ? 1ull : 0ull;
    const u64 Xv = Eq | Mv;
    Eq |= hneg;
    const u64 Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    u64 Ph = Mv | ~(Xh | Pv);
    u64 Mh = Pv & Xh;
    const int hout = (int)(Ph >> 63) - (int)(Mh >> 63);
    Ph = (Ph << 1) | hpos;
    Mh = (Mh << 1) | hneg;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
    return hout;
}

// score of the last real row (local row r of the last block) from the block's bottom score
SMX_HD int mine_last_row(u64 Pv, u64 Mv, int bottom, int r) {
    if (r == 63) return bottom;
    return bottom - (mine_popc(Pv >> (r + 1)) - mine_popc(Mv >> (r + 1)));
}

template <int WR> struct RegState {
    u64 P[WR > 0 ? WR : 1], M[WR > 0 ? WR : 1];
    int S[WR > 0 ? WR : 1];
    SMX_HD u64 &p(int w) { return P[w]; }
    SMX_HD u64 &m(int w) { return M[w]; }
    SMX_HD int &s(int w) { return S[w]; }
};

struct GlobalState {   // pointers already offset to this lane; element w at [w * MINE_THREADS]
    u64 *P, *M;
    int *S;
    SMX_HD u64 &p(int w) { return P[(size_t)w * MINE_THREADS]; }
    SMX_HD u64 &m(int w) { return M[(size_t)w * MINE_THREADS]; }
    SMX_HD int &s(int w) { return S[(size_t)w * MINE_THREADS]; }
};

// The per-lane state of class WR handed to f(st): registers for WR > 0; for WR = 0 this lane's columns of a workgroup's
// scratch slice, 3 x scratch_words x MINE_THREADS words laid out [P | M | S][word][lane].  Returns what f returns.
template <int WR, typename F> SMX_HD int mine_lane_state(u64 *slice, int scratch_words, unsigned lane, F &&f) {
    if constexpr (WR > 0) {
        RegState<WR> st;
        return f(st);
    } else {
        GlobalState st{slice + lane, slice + (size_t)scratch_words * MINE_THREADS + lane,
                       reinterpret_cast<int *>(slice + (size_t)2 * scratch_words * MINE_THREADS) + lane};
        return f(st);
    }
}

// One pair: HW distance of the query (Peq of W words, padded row stride Wp) in target t[0..n).
// Returns -1 if the distance exceeds k (k < 0: no limit).  t must be 16-byte aligned and readable up to the next
// multiple of 16 bytes past n.  WR > 0: the state of W <= WR words in registers; WR = 0: any W, state in st.
template <int WR, typename State>
SMX_MINE_HD int mine_pair(State &st, const u64 *peq, const unsigned short *rowmap, int m, int W, int Wp, int k,
                          const unsigned char *t, int n) {
    if (n == 0) return m;                          // edlib: an empty target costs the whole query, whatever k is
    if (k >= 0 && n < m - k) return -1;            // an infix needs at least m - k target bytes
    int kk = (k < 0 || k > m) ? m : k;
    const int last = W - 1, rlast = (m - 1) - 64 * last;
    int L = mine_min(last, kk / 64);
    const int wend = WR > 0 ? WR : W;
    constexpr int kUnroll = WR > 0 ? WR : 1;     // the register variants unroll fully (static indices)
#pragma unroll kUnroll
    for (int w = 0; w < wend; w++) {               // column 0: D[i][0] = i
        st.p(w) = ~0ull;
        st.m(w) = 0ull;
        st.s(w) = 64 * (w + 1);
    }
    int best = -1;
    const mine_u4 *t16 = reinterpret_cast<const mine_u4 *>(t);
    mine_u4 chunk = mine_u4_zero();
    for (int j = 0; j < n; j++) {
        if ((j & 15) == 0) chunk = t16[j >> 4];    // 16 target bytes per load (targets are 16-byte aligned, padded)
        const int jj = j & 15;
        const unsigned word = jj < 4 ? chunk.x : jj < 8 ? chunk.y : jj < 12 ? chunk.z : chunk.w;
        const u64 *eqrow = peq + (size_t)rowmap[(word >> (8 * (jj & 3))) & 0xffu] * Wp;
        int h = 0, nl = 0, sprev = 0;
        bool ext = false;
#pragma unroll kUnroll
        for (int w = 0; w < wend; w++) {
            if (w > L + 1 || w > last) break;
            if (w == L + 1) {                       // band extension: only if the bottom of L was <= k last column
                if (!ext) break;
                st.p(w) = ~0ull;
                st.m(w) = 0ull;
                st.s(w) = sprev + 64;
            }
            u64 Pv = st.p(w), Mv = st.m(w);
            const int sp = st.s(w);
            h = mine_step(eqrow[w], Pv, Mv, h);
            st.p(w) = Pv;
            st.m(w) = Mv;
            st.s(w) = sp + h;
            if (w == L) { sprev = sp; ext = sp <= kk; }
            if (sp + h < kk + 64) nl = w;          // the deepest block that may hold a cell <= k
            if (w == last) {
                const int v = mine_last_row(Pv, Mv, sp + h, rlast);
                if (v <= kk) { best = v; kk = v; }
            }
        }
        L = nl;
    }
    return best;
}

// What one pair contributes to its target's best identity: 1 - d / m in IEEE double (the reference's expression), or 0
// where the pair does not count (d = -1, identity below min_identity, identity 0).  The best of a target is the
// largest contribution over its queries; a non-negative double orders like its 64-bit pattern.
SMX_HD double mine_identity(int d, int m, double min_identity) {
    if (d == -1) return 0.0;
    const double identity = 1.0 - (double)d / (double)m;
    return (identity >= min_identity && identity > 0.0) ? identity : 0.0;
}

}  // namespace smx

#endif  // SMX_MINE_CORE_H
