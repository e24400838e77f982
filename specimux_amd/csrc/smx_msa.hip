// smx_msa.hip -- the kernels of one smx_msa call: msa_tips_kernel writes the one-hot profiles of the
// tips; then, level by level of the guide tree, msa_merge_kernel aligns the two children of every merge of the launch,
// one workgroup per merge; msa_rows_kernel, once the root's length is known, composes every tip's maps into its row.
//
// The arithmetic is smx_msa_core.h's.  Plain launches on the call's stream and nothing else: no workgroup ever waits
// for another one, the order of the launches on the stream is the only synchronisation between workgroups.  Inside a
// workgroup the waves hand rows to one another through global memory across __syncthreads(): the workgroup's waves
// share one CU and its vector cache, and the barrier orders their accesses.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_internal.h"
#include "smx_msa_core.h"

namespace smx {

__device__ __forceinline__ uint64_t msa_shfl_up(uint64_t v, unsigned d) {
    return (uint64_t)__shfl_up((unsigned long long)v, d, 64);
}
__device__ __forceinline__ uint64_t msa_shfl(uint64_t v, int lane) { return (uint64_t)__shfl((unsigned long long)v, lane, 64); }

// One workgroup per tip, a thread per base
__global__ __launch_bounds__(MSA_TIPS_THREADS) void msa_tips_kernel(const unsigned char *__restrict__ bytes,
                                                                    const uint64_t *__restrict__ doff,
                                                                    const uint64_t *__restrict__ prof_off,
                                                                    MsaCol *__restrict__ prof) {
    const uint32_t tip = blockIdx.x;
    const uint64_t at = doff[tip], len = doff[tip + 1] - at;
    MsaCol *out = prof + prof_off[tip];
    for (uint64_t k = threadIdx.x; k < len; k += MSA_TIPS_THREADS) out[k] = msa_tip_col(bytes[at + k]);
}

// One workgroup per merge of the launch; three phases, a __syncthreads() between them.
//
// 1  Forward.  A wave owns a band of 64 rows, lane r the row i = 64 band + r + 1; at step s of the band the lane computes
//    the column j = s - r + 1.  D[i-1][j] is the score lane r - 1 left one step earlier (one shuffle), D[i-1][j-1] the one
//    it left two steps earlier (the last shuffle's result), D[i][j-1] the lane's own.  a's column stays in registers.  The
//    lane collects 16 direction codes into a word and stores it itself.  Lane 63's row goes to `row`, Lb + 1 scores that
//    the band below reads as its top row -- 64 columns at the head of every block of 64 steps, handed to lane 0 by a
//    broadcast -- and overwrites in turn: the one array serves every band.  The workgroup's waves take consecutive bands,
//    each MSA_LAG blocks behind the one above, one barrier per block: the band above writes the column c in its block
//    (c + 62) / 64, the band below reads it in its block (c - 1) / 64, two blocks later on the workgroup's clock, and
//    writes it itself only after that.  Band 0's top row is the running sum of b's gap costs, kept by lane 0.
// 2  Walk back.  Thread 0 walks; the workgroup stages the tile of direction words it is in (64 rows x 16 words) into LDS
//    first, so that no step waits for global memory.  Ops are written from the end of the La + Lb bytes of `ops`.
// 3  Build.  Thread x takes the ops [x c, (x + 1) c); a scan of the threads' counts of a-columns and b-columns gives
//    where its first op reads a and b; it writes its new columns and the two maps' entries.  Thread 0 writes len_t.
// prof is read (the children) and written (the new node) at different columns: no __restrict__ on it.
__global__ __launch_bounds__(MSA_MERGE_THREADS) void msa_merge_kernel(const MsaMergeDev *__restrict__ recs, uint32_t X, uint32_t G,
                                                                      MsaCol *prof, uint16_t *__restrict__ maps, uint32_t *tb_all,
                                                                      uint8_t *ops_all, uint64_t *row_all,
                                                                      uint32_t *__restrict__ lens, uint64_t *__restrict__ costs,
                                                                      unsigned long long *__restrict__ phase) {
    __shared__ uint32_t s_tile[MSA_TILE_ROWS * MSA_TILE_WORDS];
    __shared__ uint32_t s_state[3];
    __shared__ uint32_t s_scan[2][MSA_MERGE_THREADS];
    const MsaMergeDev R = recs[blockIdx.x];
    const uint32_t La = R.La, Lb = R.Lb, na = R.na, nb = R.nb;
    const MsaCol *pa = prof + R.prof_a, *pb = prof + R.prof_b;
    MsaCol *po = prof + R.prof_out;
    uint32_t *tb = tb_all + R.tb;
    uint8_t *ops = ops_all + R.ops;
    uint64_t *row = row_all + R.row;
    const uint32_t W16 = msa_tb_words(Lb);
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const MsaCol zero = {{0, 0, 0, 0, 0, 0, 0, 0}};
    // SMX_MSA_PHASE_TIMING: thread 0 leaves the wall clock at the start, after each of the two barriers and at the end
    const bool timed = phase != nullptr && tid == 0;
    if (timed) phase[4u * blockIdx.x] = wall_clock64();

    // ---- 1: forward
    const uint32_t nbands = (La + 63u) / 64u, nsteps = Lb + 63u, nblocks = (nsteps + 63u) / 64u;
    const uint32_t wact = nbands < MSA_WAVES ? nbands : MSA_WAVES;
    const uint32_t ticks = nblocks + MSA_LAG * (wact - 1u);
    for (uint32_t band0 = 0; band0 < nbands; band0 += wact) {
        const uint32_t band = band0 + wave;
        const bool valid = wave < wact && band < nbands;         // uniform over the wave
        const uint32_t i = band * 64u + lane + 1u;
        const bool rowok = valid && i <= La;
        MsaCol ca = zero;
        uint32_t ra = 0, word = 0;
        uint64_t ga = 0, cur = 0, diagv = 0;
        for (uint32_t tick = 0; tick < ticks; tick++) {
            const uint32_t B = tick - MSA_LAG * wave;             // the wave's block; wraps while the wave still waits
            if (valid && tick >= MSA_LAG * wave && B < nblocks) {
                if (B == 0) {
                    if (rowok) ca = pa[i - 1u];
                    ra = na - ca.c[MSA_GAP];
                    ga = rowok ? msa_gap_cost(G, ra, nb) : 0;
                    const uint64_t top0 = band == 0 ? 0 : row[0];
                    uint64_t incl = ga;                           // D[i][0] = D[i0 - 1][0] + the gap costs of the rows down to i
                    for (unsigned d = 1; d < 64; d <<= 1) {
                        const uint64_t v = msa_shfl_up(incl, d);
                        if (lane >= d) incl += v;
                    }
                    cur = top0 + incl;
                    diagv = cur - ga;
                    word = 0;
                    if (lane == 63u) row[0] = cur;
                }
                uint64_t tv = 0;                                  // the top row's columns 64 B + 1 .. 64 B + 64, one per lane
                if (band != 0) {
                    const uint32_t c = 64u * B + lane + 1u;
                    if (c <= Lb) tv = row[c];
                }
                for (uint32_t q = 0; q < 64u; q++) {
                    const uint32_t s = 64u * B + q;
                    if (s >= nsteps) break;                       // uniform
                    const int32_t j = (int32_t)s - (int32_t)lane + 1;
                    const bool active = rowok && j >= 1 && j <= (int32_t)Lb;
                    MsaCol cb = zero;
                    if (active) cb = pb[j - 1];
                    uint64_t up = msa_shfl_up(cur, 1);
                    const uint64_t tq = msa_shfl(tv, (int)q);
                    if (active) {
                        const uint32_t rb = nb - cb.c[MSA_GAP];
                        const uint64_t gb = msa_gap_cost(G, rb, na);
                        if (lane == 0) up = band == 0 ? diagv + gb : tq;
                        uint32_t dir;
                        const uint64_t best = msa_min3(diagv + msa_pair_cost(ca, ra, cb, rb, X, G), up + ga, cur + gb, &dir);
                        diagv = up;
                        cur = best;
                        const uint32_t jj = (uint32_t)j - 1u;
                        word |= dir << (2u * (jj & 15u));
                        if ((jj & 15u) == 15u || (uint32_t)j == Lb) {
                            tb[(uint64_t)(i - 1u) * W16 + (jj >> 4)] = word;
                            word = 0;
                        }
                        if (lane == 63u) row[j] = best;
                        if (i == La && (uint32_t)j == Lb) costs[R.t] = best;
                    }
                }
            }
            __syncthreads();
        }
    }

    // ---- 2: walk back
    if (timed) phase[4u * blockIdx.x + 1u] = wall_clock64();
    if (tid == 0) { s_state[0] = La; s_state[1] = Lb; s_state[2] = La + Lb; }
    __syncthreads();
    for (;;) {
        uint32_t i = s_state[0], j = s_state[1];
        if (i == 0 || j == 0) break;                              // uniform
        const uint32_t r0 = i >= MSA_TILE_ROWS ? i - (MSA_TILE_ROWS - 1u) : 1u, wh = (j - 1u) >> 4;
        const uint32_t wl = wh >= MSA_TILE_WORDS - 1u ? wh - (MSA_TILE_WORDS - 1u) : 0u;
        const uint32_t nrows = i - r0 + 1u, nw = wh - wl + 1u;
        for (uint32_t x = tid; x < nrows * MSA_TILE_WORDS; x += MSA_MERGE_THREADS) {
            const uint32_t r = x / MSA_TILE_WORDS, k = x % MSA_TILE_WORDS;
            if (k < nw) s_tile[x] = tb[(uint64_t)(r0 + r - 1u) * W16 + wl + k];
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t pos = s_state[2];
            while (i >= r0 && j > 0 && ((j - 1u) >> 4) >= wl) {
                const uint32_t w = s_tile[(i - r0) * MSA_TILE_WORDS + ((j - 1u) >> 4) - wl];
                const uint32_t d = (w >> (2u * ((j - 1u) & 15u))) & 3u;
                ops[--pos] = (uint8_t)d;
                if (d != MSA_LEFT) i--;
                if (d != MSA_UP) j--;
            }
            s_state[0] = i; s_state[1] = j; s_state[2] = pos;
        }
        __syncthreads();
    }
    // the edge: i ups at j = 0, or j lefts at i = 0
    const uint32_t ei = s_state[0], ej = s_state[1], epos = s_state[2], edge = ei + ej;
    for (uint32_t x = tid; x < edge; x += MSA_MERGE_THREADS) ops[epos - 1u - x] = (uint8_t)(ei ? MSA_UP : MSA_LEFT);
    __syncthreads();

    // ---- 3: build
    if (timed) phase[4u * blockIdx.x + 2u] = wall_clock64();
    const uint32_t start = epos - edge, len = La + Lb - start, per = msa_chunk(len);
    const uint32_t p0 = tid * per < len ? tid * per : len, p1 = p0 + per < len ? p0 + per : len;
    uint32_t cnt = 0;                                             // a-columns in the high half, b-columns in the low one
    for (uint32_t p = p0; p < p1; p++) {
        const uint32_t op = ops[start + p];
        cnt += (op != MSA_LEFT ? 0x10000u : 0u) + (op != MSA_UP ? 1u : 0u);
    }
    s_scan[0][tid] = cnt;
    __syncthreads();
    unsigned src = 0;
    for (unsigned d = 1; d < MSA_MERGE_THREADS; d <<= 1) {
        s_scan[src ^ 1u][tid] = s_scan[src][tid] + (tid >= d ? s_scan[src][tid - d] : 0u);
        __syncthreads();
        src ^= 1u;
    }
    const uint32_t excl = s_scan[src][tid] - cnt;
    uint32_t ia = excl >> 16, ib = excl & 0xffffu;
    uint16_t *map_a = maps + R.map_a, *map_b = maps + R.map_b;
    for (uint32_t p = p0; p < p1; p++) {
        const uint32_t op = ops[start + p];
        const MsaCol a = op != MSA_LEFT ? pa[ia] : zero, b = op != MSA_UP ? pb[ib] : zero;
        po[p] = msa_new_col(op, a, b, na, nb);
        if (op != MSA_LEFT) map_a[ia++] = (uint16_t)p;
        if (op != MSA_UP) map_b[ib++] = (uint16_t)p;
    }
    if (tid == 0) lens[R.t] = len;
    if (timed) phase[4u * blockIdx.x + 3u] = wall_clock64();
}

// One workgroup per tip: the row filled with '-' in LDS, a thread per base following parent[] and the maps to the root
__global__ __launch_bounds__(MSA_ROWS_THREADS) void msa_rows_kernel(const unsigned char *__restrict__ bytes,
                                                                    const uint64_t *__restrict__ doff,
                                                                    const uint32_t *__restrict__ parent,
                                                                    const uint64_t *__restrict__ map_off,
                                                                    const uint16_t *__restrict__ maps, uint32_t n_cols,
                                                                    uint8_t *__restrict__ rows) {
    __shared__ uint8_t s_row[SMX_MSA_MAX_COLS];
    const uint32_t tip = blockIdx.x;
    for (uint32_t c = threadIdx.x; c < n_cols; c += MSA_ROWS_THREADS) s_row[c] = (uint8_t)'-';
    __syncthreads();
    const uint64_t at = doff[tip], len = doff[tip + 1] - at;
    for (uint64_t k = threadIdx.x; k < len; k += MSA_ROWS_THREADS) {
        uint32_t col = (uint32_t)k, node = tip;
        for (uint32_t p = parent[node]; p != MSA_NONE; p = parent[node]) {
            col = maps[map_off[node] + col];
            node = p;
        }
        if (col < n_cols) s_row[col] = bytes[at + k];
    }
    __syncthreads();
    uint8_t *out = rows + (uint64_t)tip * n_cols;
    for (uint32_t c = threadIdx.x; c < n_cols; c += MSA_ROWS_THREADS) out[c] = s_row[c];
}

}  // namespace smx

extern "C" int smx_launch_msa_tips(void *stream, const unsigned char *d_bytes, const uint64_t *d_doff, uint32_t n,
                                   const uint64_t *d_prof_off, void *d_prof) {
    using namespace smx;
    if (n == 0 || n > (uint32_t)SMX_MSA_MAX_N) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(msa_tips_kernel, dim3(n), dim3(MSA_TIPS_THREADS), 0, (hipStream_t)stream, d_bytes, d_doff, d_prof_off,
                       reinterpret_cast<MsaCol *>(d_prof));
    return (int)hipGetLastError();
}

extern "C" int smx_launch_msa_merge(void *stream, const void *d_recs, uint32_t count, uint32_t X, uint32_t G, void *d_prof,
                                    uint16_t *d_maps, uint32_t *d_tb, uint8_t *d_ops, uint64_t *d_row, uint32_t *d_lens,
                                    uint64_t *d_costs, unsigned long long *d_phase) {
    using namespace smx;
    if (count == 0 || count > (uint32_t)SMX_MSA_MAX_N) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(msa_merge_kernel, dim3(count), dim3(MSA_MERGE_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const MsaMergeDev *>(d_recs), X, G, reinterpret_cast<MsaCol *>(d_prof), d_maps, d_tb,
                       d_ops, d_row, d_lens, d_costs, d_phase);
    return (int)hipGetLastError();
}

extern "C" int smx_launch_msa_rows(void *stream, const unsigned char *d_bytes, const uint64_t *d_doff, uint32_t n,
                                   const uint32_t *d_parent, const uint64_t *d_map_off, const uint16_t *d_maps, uint32_t n_cols,
                                   uint8_t *d_rows) {
    using namespace smx;
    if (n == 0 || n > (uint32_t)SMX_MSA_MAX_N || n_cols == 0 || n_cols > (uint32_t)SMX_MSA_MAX_COLS) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(msa_rows_kernel, dim3(n), dim3(MSA_ROWS_THREADS), 0, (hipStream_t)stream, d_bytes, d_doff, d_parent,
                       d_map_off, d_maps, n_cols, d_rows);
    return (int)hipGetLastError();
}
