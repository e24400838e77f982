// smx_internal.h -- device-side view of the panel, shared by the .hip files and the host files (smx_host.h).
#ifndef SMX_INTERNAL_H
#define SMX_INTERNAL_H
#include <stddef.h>
#include <stdint.h>
#include "smx.h"
#include "smx_prescan_core.h"
#include "smx_mine_core.h"
#include "smx_inner_core.h"

// LDS a CU of gfx950 gives to workgroups (in 512-byte granules): measured, tools/ubench/lds_residency.hip
#define SMX_LDS_POOL ((size_t)159744)

namespace smx {

// Text alphabet of the kernels: 16 codes.  Code 15 ("other") never matches any pattern character.
// Order matters only for the LUTs built in smx_panel.cpp.
static const char kCodeChars[16] = {'A', 'C', 'G', 'T', 'N', 'R', 'Y', 'K', 'M', 'S', 'W', 'B', 'D', 'H', 'V', 0};

// One specimen as the scorer needs it, 32 bytes: two of these tables -- per (b1, b2) barcode pair the FIRST specimen in
// file order (spec = -1: none), per specimen its own record -- so that specimen_exact is one load in the usual case.
struct SpecRec {
    unsigned long long p1m, p2m;   // forward / reverse primers the specimen is registered with (bit = primer index)
    int spec, next, pool, pad;     // specimen index, next specimen with the same barcode pair (-1: none), its pool
};

// All pointers are DEVICE pointers (one allocation, see smx_panel.cpp).  Passed to kernels by value.
struct DevPanel {
    int NP, NB, NS, NPAIR;
    int n_pbc;        // total length of the per-primer barcode lists
    int S;            // search_len
    int wstride;      // bytes per read in the window buffer
    int kidx;         // max_dist_index
    int bmax;         // Specimens.b_length()
    int pfmin;        // prefilter min length, 0 = off
    int preorient, trim, derep, minlen, maxlen;
    int maxB;         // max barcodes per primer
    int need_starts;  // HW start locations required (trim primers / tails)
    const unsigned long long *ppeq;   // NP*16 : bit i of ppeq[p*16+c] = eq(primer_rc[i], code c)
    const unsigned long long *prpeq;  // NP*16 : same for the reversed pattern
    const unsigned *bpeq;             // NB*16
    const unsigned char *lut;         // [0,256): ASCII -> code; [256,512): ASCII -> code of the complement
    const int *pm, *pk, *pdir, *pfidx;    // per primer: pattern length, k_p, direction, file index
    const int *pbc_off, *pbc;             // per primer barcode list (global barcode indices)
    const int *bm;                        // per barcode length
    const int *pair_f, *pair_r, *pair_pool;
    const SpecRec *pairrec;               // NB*NB: the first specimen (file order) with (b1, b2), as a whole record; spec = -1: none
    const SpecRec *specrec;               // per specimen: its record (next = the following specimen with the same barcode pair)
    // bit-sliced barcode scan (lean mode): all barcodes one length bs_m <= 16, k <= 7.
    // bs_re[((p * 16 + row) * 16 + code) * MBW + w] = bitmask over primer p's barcode list: barcode_rc[row] eq code
    int bs_ok, bs_m;
    int n_bstab;              // distinct per-primer tables in bs_re (primers with the same barcode list share one)
    const int *bs_tab;        // per primer: its table
    int cap_hits, cap_ents;   // test hook (SMX_TEST_CAPS=h,e): force small barcode rounds; 0 = default sizing
    int no_sp;                // SMX_NO_SPECIALISE (bit 0) / SMX_NO_SPECIALISE_NP (bit 1)
    int tile_codes;           // the prescan hands tile-major codes on (DemuxAux::tiled of every launch): the two-primer kernel has that layout compiled in
    const unsigned *bs_re;
    unsigned long long *dbg_phase;        // SMX_PHASE_TIMING=1: [grid][16] cycle sums per phase (diagnostic build-in)
};

// Compact mode and the redo launch behind it (smx_demux_tile.h, demux_kernel).
struct DemuxAux {
    const unsigned *match;   // prescan match words [tile of 1024 reads][alignment][32-read group]; compact mode only
    unsigned *ovf_list;      // compact launch: the tiles it could not hold (appended); redo launch: the tiles to process
    int nitems;              // > 0: compact mode, this many per-alignment records per tile (<= 256)
    int redo;                // 1: this launch processes the reads of ovf_list's tiles (Rc reads each) and nothing else
    int Rc;                  // reads per tile of the compact launch
    int chain;               // 1: another launch of this batch follows: the extra-record and overflow counters stay
    const unsigned *codes2;  // prescan: 2-bit codes per read in DP order (smx_prescan_core.h codes2_from_piece); nullptr: encode from ASCII
    const uint8_t *naflag;   // prescan: per read, 1 = a window holds something other than upper-case ACGT (ASCII path for that read)
    int tiled;               // layout of codes2: 0 row-major per read (codes2_word), 1 tile-major (tilecodes_word)
};

// One launch mode's tile: reads per tile, its LDS image, and the resident workgroups per CU the grid counts on.
struct TilePlan { int R = 0; size_t lds = 0; int blocks_per_cu = 1; };

// One batch as smx_batch_run_device receives it (the ten buffers of include/smx.h), and where it runs.
struct DemuxBatch {
    const uint8_t *windows; const int32_t *lens; uint32_t n_reads;
    smx_op *ops, *extra; uint32_t extra_cap, *n_extra; uint64_t *counts;
    smx_hit *hits; int8_t *bdist;   // optional dumps
    void *stream;
    unsigned *tile_counter;         // the stream's launch counters on this panel
    const unsigned *pre; uint32_t npad;   // prescan flag words of the batch (nullptr: no prescan), npad reads per (alignment, chunk)
};

// specimine (smx_mine.hip): chunks of one query x up to MINE_THREADS (smx_mine_core.h) targets, one target per lane
#define MINE_LDS_HEAD 192   // u64 words before the Peq table: byte -> row map (512 B) + byte presence flags (1 KiB)

struct MineJobDev {   // one smx_mine_job with its output offsets
    uint32_t q0, nq, t0, nt;
    uint64_t dist_off, best_off;
    double min_identity;
};

struct MinePair {     // one (job, query) pair, ceil(nt / MINE_THREADS) target chunks
    uint32_t job;     // index into the MineJobDev array
    uint32_t q;       // query index
    int32_t k;        // max distance of the query (< 0: none)
    uint32_t pad;
};

// clusters (smx_pairs.hip): all pairs i < j of a job's reads; chunks as in specimine, aligned in j
struct PairsJobDev {  // one smx_pairs_job with its output offset (int32 distances or uint32 adjacency words)
    uint32_t r0, n;
    uint64_t out_off;
};

struct PairsRow {     // row i of a job's triangle: ceil(n / MINE_THREADS) - (i + 1) / MINE_THREADS target chunks
    uint32_t job;     // index into the PairsJobDev array
    uint32_t read;    // the query: read r0 + i
};

// consensus (smx_cons.hip): a job's draft against its member reads [r0, r0 + n); chunks of MINE_THREADS members
struct ConsJobDev {
    uint32_t draft, r0, n;
    uint32_t B;           // history slots per column: the most any member's band needs (smx_cons_core.h cons_band_blocks)
    uint64_t rows_off;    // the job's n x (m + 1) row words
    uint64_t dist_off;    // its n distances
    uint64_t votes_off;   // its (m + 1) x SMX_CONS_VOTE_WORDS vote words
};
// errors (smx_profile.hip): a workgroup takes SMX_PROFILE_BLOCK_MEMBERS members of a job, each of its waves
// SMX_PROFILE_WAVE_MEMBERS of them; the plan (smx_cons_plan.h cons_plan_profile) sizes the grid by the former
constexpr uint32_t SMX_PROFILE_WAVE_MEMBERS = 4, SMX_PROFILE_BLOCK_MEMBERS = 16;

// inner scan (smx_inner.hip): one chunk of whole reads and one word-width class of patterns.  Device pointers.
struct InnerArgs {
    const void *peq;               // [pass][16 codes][G] match words, 32 or 64 bits wide
    const int *pm, *pk, *jmap;     // [pass * G]: pattern length, threshold (-1: padding slot), index in the call (-1: padding)
    const unsigned char *lut;      // 256: read byte -> code
    const mine_u4 *bases;          // the chunk's reads back to back, readable to the end of the last byte's 16-byte word
    const uint64_t *roff;          // n_reads + 1 byte offsets into bases
    const uint32_t *unit_read;     // per unit: its read
    const uint32_t *ustart;        // n_reads + 1: first unit of each read
    uint32_t n_units;
    int Q, H, margin, PL, lead;
    uint32_t *recs;                // n_units * Q records of inner_rec_words(H) words
};

}  // namespace smx

extern "C" {
// primer prescan (smx_prescan.hip)
size_t smx_prescan_lds_bytes(int S, int tile);
int smx_launch_prescan(const smx::PreDesc *D, int mr, int nx, int grid_t, size_t lds_t, int grid_d, void *stream,
                       const uint8_t *d_windows, const int32_t *d_lens, uint32_t n_reads, int stride, unsigned *d_planes,
                       unsigned *d_out, unsigned *d_match, void *ev_mid, unsigned *d_codes2, uint8_t *d_naflag);
int smx_prescan_set_lds_limit(size_t bytes);
int smx_prescan_occupancy(int S, int mr, int nx, int tile, size_t lds_t, int *blocks_t, int *blocks_d);
int smx_prescan_transpose_threads(int S);
// alignment kernels (smx_align.hip)
int smx_launch_align(void *stream, const unsigned long long *d_peq, const unsigned long long *d_rpeq, int m,
                     const unsigned char *d_tcodes, int n, int k, int mode, int *d_dist, unsigned char *d_endflag,
                     int *d_starts);
int smx_launch_align_batch(void *stream, const unsigned long long *d_qpeq, const int *d_qlen, const unsigned *d_qidx,
                           const unsigned char *d_tcodes, const unsigned long long *d_toff, const int *d_k,
                           const unsigned char *d_modes, unsigned n, unsigned char *d_ws, int *d_dist, int *d_nloc,
                           int *d_starts, int *d_ends, unsigned cap);
// specimine (smx_mine.hip); wr = register words per lane (1, 2, 4, 8, 16) or 0 = state in d_scratch; pairs[0..n_pairs)
// with chunk_start[0..n_pairs] (prefix sum of their target chunks, nonzero each); workgroup b takes chunks
// [b * per_block, (b + 1) * per_block), grid * per_block >= the chunk count.  dist = 0: d_out holds the 64-bit patterns
// of the non-negative best identities (zeroed by the caller); dist = 1: d_out holds the int32 distances, job j's
// nq x nt row-major at its dist_off
int smx_launch_mine(void *stream, int wr, int dist, const unsigned char *d_q, const uint64_t *d_qoff, const unsigned char *d_t,
                    const uint64_t *d_toff, const int32_t *d_tlen, const void *d_pairs, const uint64_t *d_chunk_start,
                    uint32_t n_pairs, const void *d_jobs, int grid, uint64_t per_block, size_t lds_bytes, void *d_out,
                    unsigned long long *d_scratch, int scratch_words);
// clusters (smx_pairs.hip); wr, grid, per_block, d_scratch as for smx_launch_mine.  d_bytes / d_off / d_len: the reads
// as 16-byte aligned padded copies; d_k: the limit per read; rows[0..n_rows) with chunk_start[0..n_rows] (nonzero
// each).  dist = 1: d_out holds int32 distances, job j's packed upper triangle at its out_off; dist = 0: d_out holds
// the adjacency words (zeroed by the caller), the kernel writes the upper triangle of job j's n x ceil(n / 32) matrix
int smx_launch_pairs(void *stream, int wr, int dist, const unsigned char *d_bytes, const uint64_t *d_off, const int32_t *d_len,
                     const int32_t *d_k, const void *d_rows, const uint64_t *d_chunk_start, uint32_t n_rows,
                     const void *d_jobs, int grid, uint64_t per_block, size_t lds_bytes, void *d_out,
                     unsigned long long *d_scratch, int scratch_words);
// consensus (smx_cons.hip); wr, grid, per_block, d_scratch, d_bytes / d_off / d_len / d_k as for smx_launch_pairs.
// jobs[0..n_jobs) (ConsJobDev, n > 0 each) with chunk_start[0..n_jobs]; workgroup b keeps its history in entries
// [b * hist_slice * MINE_THREADS, (b + 1) * hist_slice * MINE_THREADS) of d_hist_pm (16 bytes each) and d_hist_s.
int smx_launch_cons_align(void *stream, int wr, const unsigned char *d_bytes, const uint64_t *d_off, const int32_t *d_len,
                          const int32_t *d_k, const void *d_jobs, const uint64_t *d_chunk_start, uint32_t n_jobs, int grid,
                          uint64_t per_block, size_t lds_bytes, uint32_t *d_rows, int32_t *d_dist, void *d_hist_pm,
                          int *d_hist_s, uint64_t hist_slice, unsigned long long *d_scratch, int scratch_words);
// the votes of jobs[0..n_jobs) (any n) from the rows and distances the alignment left; max_words = the largest m + 1
int smx_launch_cons_vote(void *stream, const int32_t *d_len, const void *d_jobs, uint32_t n_jobs, uint32_t max_words,
                         const uint32_t *d_rows, const int32_t *d_dist, uint32_t *d_votes, uint32_t *d_aligned);
// variants (smx_phase.hip), after the two launches above on the same stream: the sites of jobs[0..n_jobs) from d_votes and
// d_aligned into d_sites (smx_cons_site, max_sites per job) / d_n_sites / d_n_qualified, the allele planes from d_rows and
// d_dist into d_planes (job j's max_sites x 2 x ceil(n / 64) words at planes_off[j]; max_plane_words = the largest
// ceil(n / 64)), and the max_sites x max_sites x 4 link words per job into d_link.  Every table is written in full
int smx_launch_cons_phase(void *stream, const int32_t *d_len, const void *d_jobs, uint32_t n_jobs, const uint32_t *d_rows,
                          const int32_t *d_dist, const uint32_t *d_votes, const uint32_t *d_aligned, uint32_t min_permille,
                          uint32_t min_reads, uint32_t max_sites, uint32_t max_plane_words, const uint64_t *d_planes_off,
                          void *d_sites, uint32_t *d_n_sites, uint32_t *d_n_qualified, uint64_t *d_planes, uint32_t *d_link);
// support (smx_resample.hip), after smx_launch_cons_align and smx_launch_cons_vote on the same stream: per (job, level,
// column) the 64 replicates that keep the column, from d_rows, d_dist and the n_levels x level_stride mask words (job j's
// members at member_off[j] of every level), into d_agree (job j's n_levels x (m + 1) words at agree_off[j]) and the
// replicates' voters into d_sub_aligned ([job][level][64]).  max_words = the largest m + 1.  Every word is written
int smx_launch_cons_resample(void *stream, const unsigned char *d_bytes, const uint64_t *d_off, const int32_t *d_len,
                             const void *d_jobs, uint32_t n_jobs, uint32_t n_levels, uint32_t max_words, const uint32_t *d_rows,
                             const int32_t *d_dist, const uint64_t *d_masks, const uint64_t *d_member_off,
                             const uint64_t *d_agree_off, uint64_t level_stride, uint64_t *d_agree, uint32_t *d_sub_aligned);
// errors (smx_profile.hip), after smx_launch_cons_align and smx_launch_cons_vote on the same stream: per member its
// SMX_PROFILE_MEMBER_WORDS counts into d_per_member (job j's members from dist_off on), per job its SMX_PROFILE_JOB_WORDS table
// words added into d_tables (zeroed by the caller), from d_rows, d_dist, the drafts' bytes and the quality bytes d_quals with
// their n_reads + 1 offsets d_qoff (the caller's layout, not the padded one).  max_members = the largest job's n
int smx_launch_cons_profile(void *stream, const unsigned char *d_bytes, const uint64_t *d_off, const int32_t *d_len,
                            const void *d_jobs, uint32_t n_jobs, uint32_t max_members, const uint32_t *d_rows,
                            const int32_t *d_dist, const unsigned char *d_quals, const uint64_t *d_qoff,
                            uint32_t *d_per_member, uint32_t *d_tables);
// crosstalk (smx_nearest.hip); wr, grid, per_block, d_scratch, d_bytes / d_off / d_len / d_k as for smx_launch_pairs;
// d_group: the group per sequence.  runs[0..n_runs) (NearestRun over the class's ref list d_refs) with
// chunk_start[0..n_runs] (nonzero each).  dist = 1: d_dist holds int32 distances, job j's nq x nt at its dist_off;
// dist = 0: d_best_own / d_best_other hold the keys (filled with 0xFF bytes by the caller), job j's nt at its best_off
int smx_launch_nearest(void *stream, int wr, int dist, const unsigned char *d_bytes, const uint64_t *d_off, const int32_t *d_len,
                       const int32_t *d_k, const uint32_t *d_group, const uint32_t *d_refs, const void *d_runs,
                       const uint64_t *d_chunk_start, uint32_t n_runs, const void *d_jobs, int grid, uint64_t per_block,
                       size_t lds_bytes, unsigned long long *d_best_own, unsigned long long *d_best_other, int32_t *d_dist,
                       unsigned long long *d_scratch, int scratch_words);
// identify (smx_hits.hip); wr, grid, per_block, d_scratch, d_bytes / d_off / d_len / d_k as for smx_launch_pairs.
// recs[0..n_recs) (HitsRec, smx_hits_core.h, windows of the order array d_ord) with chunk_start[0..n_recs] (nonzero
// each).  dist = 1: d_dist holds int32 distances (filled with -1 by the caller), job j's nq x nt at its dist_off;
// dist = 0: d_keys holds K keys per query (filled with 0xFF bytes by the caller), job j's rows from its row_off
int smx_launch_hits(void *stream, int wr, int dist, const unsigned char *d_bytes, const uint64_t *d_off, const int32_t *d_len,
                    const int32_t *d_k, const uint32_t *d_ord, const void *d_recs, const uint64_t *d_chunk_start,
                    uint32_t n_recs, const void *d_jobs, int grid, uint64_t per_block, size_t lds_bytes, int K,
                    unsigned long long *d_keys, int32_t *d_dist, unsigned long long *d_scratch, int scratch_words);
// bimera (smx_reach.hip).  d_bytes / d_doff: the padded sequences forwards at [0, n_seqs) and reversed at
// [n_seqs, 2 n_seqs) (smx_reach_plan.h reach_sequences); d_len / d_weight / d_need per sequence.  recs[0..n_recs)
// (ReachRec, smx_reach_core.h) with chunk_start[0..n_recs] (nonzero each); grid, per_block as for smx_launch_mine.
// matrix = 0: d_keys holds 2 x (E + 1) x 2 keys per query (filled with 0xFF bytes by the caller), job j's rows from its
// row_off; matrix = 1: d_values holds 2 x (E + 1) values per pair (filled with 0xFF bytes), job j's from its mat_off
int smx_launch_reach(void *stream, int matrix, const unsigned char *d_bytes, const uint64_t *d_doff, const int32_t *d_len,
                     const uint32_t *d_weight, const uint32_t *d_need, const void *d_recs, const uint64_t *d_chunk_start,
                     uint32_t n_recs, const void *d_jobs, int grid, uint64_t per_block, int E, uint32_t n_seqs,
                     unsigned long long *d_keys, uint32_t *d_values);
// tree (smx_nj.hip): every launch of one call, 3 < n <= SMX_NJ_MAX_N, enqueued without a wait in between: the init launch
// over the n (n - 1) / 2 entries of d_tri, then for each merge t = 0 .. n - 4 the row minima and the join.  d_d: n x n
// doubles; d_r, d_best_q: n doubles; d_node, d_best_hi: n uint32; d_merges: n - 3 smx_nj_merge.  Every entry a launch
// reads was written by an earlier launch of the same call.  Afterwards the slots 0, 1, 2 of d_d and d_node are the last three
int smx_launch_nj(void *stream, const int32_t *d_tri, uint32_t n, double *d_d, double *d_r, uint32_t *d_node,
                  double *d_best_q, uint32_t *d_best_hi, void *d_merges);
// msa (smx_msa.hip).  d_bytes / d_doff: the n sequences back to back and their n + 1 offsets from 0.  tips: the one-hot
// profiles of the tips, tip i's at the column d_prof_off[i] of d_prof (16 bytes a column).  merge: the `count` merges of one
// launch (MsaMergeDev, smx_msa_core.h, offsets into d_prof, d_maps and the launch's scratch d_tb / d_ops / d_row), all of one
// level of the tree: each reads its children's profiles, which earlier launches wrote, and writes the new node's profile,
// its children's maps, lens[t] and costs[t].  rows: n rows of n_cols bytes from the maps, d_parent (MSA_NONE: the root)
// and d_map_off per node.  d_phase (may be null): 4 wall-clock reads per merge of the launch, thread 0's, at the start, after
// the forward phase, after the walk and at the end (SMX_MSA_PHASE_TIMING)
int smx_launch_msa_tips(void *stream, const unsigned char *d_bytes, const uint64_t *d_doff, uint32_t n,
                        const uint64_t *d_prof_off, void *d_prof);
int smx_launch_msa_merge(void *stream, const void *d_recs, uint32_t count, uint32_t X, uint32_t G, void *d_prof, uint16_t *d_maps,
                         uint32_t *d_tb, uint8_t *d_ops, uint64_t *d_row, uint32_t *d_lens, uint64_t *d_costs,
                         unsigned long long *d_phase);
int smx_launch_msa_rows(void *stream, const unsigned char *d_bytes, const uint64_t *d_doff, uint32_t n, const uint32_t *d_parent,
                        const uint64_t *d_map_off, const uint16_t *d_maps, uint32_t n_cols, uint8_t *d_rows);
// inner scan (smx_inner.hip): the scan over A->n_units units x npass passes of G (4 or 8) patterns, w64 = 64-bit words;
// then one merge launch over n_reads x A->Q (read, pattern) pairs once every class has left its records
int smx_launch_inner_scan(void *stream, int w64, int G, int npass, const smx::InnerArgs *A);
int smx_launch_inner_merge(void *stream, const smx::InnerArgs *A, uint32_t n_reads, uint8_t *d_nhit, int8_t *d_hit_dist,
                           int32_t *d_hit_end);
}
#endif
