/*
 * smx.h -- C ABI of libsmx.so, the MI355X (gfx950) dual-barcode demultiplexing hot path.
 *
 * The reference (joshuaowalker/specimux, pure Python) has no FFI of its own; the path this
 * library replaces sits behind these reference interfaces (paths relative to the reference repo):
 *
 *   smx_batch_run / smx_batch_run_device
 *        <- process_sequences(seq_records, parameters, specimens, args, prefilter, ...)
 *           src/specimux/demultiplex.py:108-212 (one call per read batch; callers
 *           multiprocessing_utils.py:89 and orchestration.py:513), i.e. everything below it:
 *           determine_orientation :602, find_candidate_matches :668, match_one_end :748,
 *           align_seq alignment.py:21-50 (edlib HW/SHW, IUPAC equalities constants.py:13-20),
 *           BloomPrefilter.match bloom_filter.py:176, select_best_matches :216,
 *           dereplicate_matches :262 (+ :396, :480), resolve_specimen :541,
 *           create_write_operation :30 (trim extents models.py:278-319).
 *   smx_panel_create  <- the Specimens / PrimerDatabase / MatchParameters objects that
 *           process_sequences receives (databases.py:123-275, models.py:331-338,
 *           thresholds orchestration.py:548-628), flattened into arrays by the host.
 *   smx_align         <- align_seq's edlib.align call (alignment.py:42), one alignment, for unit parity.
 *   smx_pack_windows  <- the two `search_len` end slices match_one_end / determine_orientation take
 *           (demultiplex.py:757-766, :612-624): the only bases the hot path ever reads.
 *   smx_mine_*        <- specimine.py's mine_sequences (the separate specimine tool, :197-257): batched long-read
 *           HW distances and the per-partial-read best identity.
 *   smx_pairs_*       <- nothing: the reference leaves "is this specimen one organism?" to the tools after it
 *           (DESIGN.md section 14).
 *   smx_nearest*      <- nothing: nor does it ask where a well's foreign reads came from.
 *   smx_best_hits*    <- nothing: naming a consensus from a reference FASTA is left to BLAST or a web form (DESIGN.md
 *           section 17).
 *   smx_prefix_reach* <- nothing: no tool of the reference asks whether a called sequence is a left piece of one
 *           sequence of the run and a right piece of another.
 *   smx_cons_*        <- nothing: the reference hands the consensus of a specimen to an external tool (DESIGN.md
 *           section 15), and never asks whether a cluster holds two sequences (smx_cons_phase, section 18) or how far
 *           a called sequence can be trusted (smx_cons_resample, section 20), or how noisy the reads themselves are
 *           (smx_cons_profile, section 21).
 *   smx_nj            <- nothing: the reference builds no tree of a run's sequences.
 *   smx_msa           <- nothing: the reference aligns no run's sequences to one another.
 *   smx_inner_scan    <- nothing: the reference never looks between the two end windows.
 *   smx_counts_*      <- the parent summing (batch_total, batch_matched) (orchestration.py:203-207).
 *
 * Conventions: plain pointers and sizes only; the caller owns every buffer; no callbacks; every
 * function returns 0 on success or a negative smx_status and leaves a message for smx_last_error()
 * (thread local).  There is NO CPU fallback in this library: without a HIP device every compute
 * entry point fails with SMX_ERR_DEVICE.
 */
#ifndef SMX_H
#define SMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMX_ABI_VERSION 13   /* goes up when an existing declaration of this file changes: the binding
                              * (specimux_amd/_lib.py) refuses a library of another number.  A declaration that is only
                              * added needs no new number: the binding looks every symbol up and refuses a library that
                              * lacks one */

typedef enum {
    SMX_OK = 0,
    SMX_ERR_ARG = -1,      /* bad argument / inconsistent descriptor */
    SMX_ERR_UNSUPPORTED = -2, /* panel outside the kernel's limits (pattern > 64 nt, ...) */
    SMX_ERR_DEVICE = -3,   /* HIP error or no device */
    SMX_ERR_OVERFLOW = -4  /* the extra-record buffer was too small (retry with the reported size), or one read produced more than 65535 write operations (n_ops is 16 bits), or the statistics table filled up (smx_stats_read, smx_flank_read) */
} smx_status;

/* trim modes (constants.py:40-45) and dereplication strategies (:48-51) */
enum { SMX_TRIM_NONE = 0, SMX_TRIM_TAILS = 1, SMX_TRIM_BARCODES = 2, SMX_TRIM_PRIMERS = 3 };
enum { SMX_DEREP_NONE = 0, SMX_DEREP_BEST = 1 };
/* ResolutionType (constants.py:54-60); 0 = read dropped by the length filter (demultiplex.py:135-140) */
enum { SMX_R_FILTERED = 0, SMX_R_FULL = 1, SMX_R_PARTIAL_FWD = 2, SMX_R_PARTIAL_REV = 3,
       SMX_R_MULTIPLE = 4, SMX_R_UNKNOWN = 5, SMX_R_DEREP_FULL = 6 };

/* smx_op.flags */
#define SMX_OPF_REVERSE    0x01u /* output sequence is the reverse complement of the read (demultiplex.py:724) */
#define SMX_OPF_TRIM_EMPTY 0x02u /* trim would be empty: untrimmed record to unknown/unknown/unknown-unknown (:45-73) */
#define SMX_OPF_NO_SPECIMEN 0x04u /* full match without a specimen (the reference logs a warning, :571-575) */

/*
 * One WriteOperation (models.py:341-357) in index form; 32 bytes.  Every unfiltered read has exactly
 * one primary record ops[read]; reads with n_ops > 1 have their 2nd.. records appended to the
 * extra buffer (any order between reads, emission order within a read).
 */
typedef struct smx_op {
    int32_t sample;      /* specimen index (file order) for full matches, else -1 */
    int32_t trim_start;  /* output = oriented_sequence[trim_start:trim_end] */
    int32_t trim_end;
    int16_t pool;        /* pool index, -1 = "unknown" */
    int16_t p1;          /* forward primer index (registration order), -1 = "unknown" */
    int16_t p2;          /* reverse primer index, -1 = "unknown" */
    int16_t barcode;     /* partial matches: global barcode index of barcode_fwd_/barcode_rev_, else -1 */
    int8_t dist[4];      /* distance code p1,b1,b2,p2; -1 prints as 'X' (models.py:206-218) */
    uint8_t rtype;       /* SMX_R_* */
    uint8_t flags;       /* SMX_OPF_* */
    uint16_t n_ops;      /* number of write operations of this read (primary record only) */
    uint32_t read;       /* read index inside the batch */
} smx_op;

/*
 * Debug/parity dump of the per (read, primer, end) search results ("hit table"); end 0 = A = 3' end of the
 * reverse complement, end 1 = B = 3' end of the read.  Coordinates are the reference's
 * align_seq coordinates in that end's string (before AlignmentResult.reversed()).
 */
typedef struct smx_hit {
    int32_t first_start;  /* first optimal primer location (start, end), -1 when no match */
    int32_t first_end;
    int32_t tail_end;     /* max optimal end over all within-k barcodes (for --trim tails), -1 */
    int16_t pdist;        /* primer edit distance, -1 no match */
    int16_t nloc;         /* number of optimal primer end locations */
    int16_t bbest;        /* best barcode distance at this end, -1 none, -2 not searched (orientation pruned) */
    int16_t ntied;        /* barcodes tied at bbest */
    int16_t first_tied;   /* global barcode index of the first tied barcode (canonical order), -1 */
    int16_t flags;        /* bit 0: this alignment votes in determine_orientation (demultiplex.py:602-638; differs from
                             pdist >= 0 only for reads shorter than search_len - 1) */
} smx_hit;

/* Flattened panel; strings are concatenated ASCII with n+1 offsets. */
typedef struct smx_panel_desc {
    uint32_t abi_version;        /* SMX_ABI_VERSION */
    uint32_t n_primers;          /* Specimens._primers registration order (Q5, databases.py:151-165) */
    uint32_t n_barcodes;         /* distinct barcode strings, global list */
    uint32_t n_specimens;        /* file order */
    uint32_t n_pools;
    uint32_t n_pairs;            /* (fwd, rev) in find_candidate_matches order (demultiplex.py:699-700) */

    const char *primer_rc;       /* reverse complements (the searched patterns, models.py:27) */
    const uint32_t *primer_rc_off;   /* n_primers + 1 */
    const uint8_t *primer_dir;   /* 0 forward, 1 reverse */
    const int32_t *primer_k;     /* max_dist_primers (orchestration.py:605-614) */
    const int32_t *primer_file_index; /* order in primers.fasta (models.py:31) */
    const uint32_t *primer_bc_off;   /* n_primers + 1: CSR into primer_bc */
    const uint32_t *primer_bc;   /* global barcode indices, canonical order (Q4) */

    const char *barcode_rc;      /* reverse complements of the barcodes (demultiplex.py:782) */
    const uint32_t *barcode_rc_off;  /* n_barcodes + 1 */

    const uint32_t *pair_fwd;    /* n_pairs primer indices */
    const uint32_t *pair_rev;
    const int32_t *pair_pool;    /* get_pool_from_primers (demultiplex.py:640-665), -1 none */

    const uint32_t *spec_b1;     /* n_specimens global barcode indices */
    const uint32_t *spec_b2;
    const uint64_t *spec_p1mask; /* bit p set: primer p in the specimen's p1 list (wildcards expand) */
    const uint64_t *spec_p2mask;
    const int32_t *spec_pool;

    int32_t k_index;             /* max_dist_index */
    int32_t search_len;          /* -l */
    int32_t barcode_len_max;     /* Specimens.b_length() */
    int32_t prefilter_min_len;   /* BloomPrefilter.min_length = L - k; 0 = prefilter disabled */
    int32_t preorient;           /* 0/1 (--disable-preorient) */
    int32_t trim;                /* SMX_TRIM_* */
    int32_t dereplicate;         /* SMX_DEREP_* */
    int32_t min_length;          /* -1 off */
    int32_t max_length;          /* -1 off */
    int32_t want_starts;         /* 1: report first_start even when the trim mode does not need it (trace, --color) */
} smx_panel_desc;

typedef struct smx_panel smx_panel; /* opaque, immutable after create; holds host + device copies */

/* counts vector layout (uint64): fixed slots then one per specimen */
enum { SMX_CNT_TOTAL = 0, SMX_CNT_MATCHED = 1, SMX_CNT_FILTERED = 2, SMX_CNT_OPS_FULL = 3,
       SMX_CNT_OPS_PARTIAL = 4, SMX_CNT_OPS_UNKNOWN = 5, SMX_CNT_MULTI_OP_READS = 6,
       SMX_CNT_OVERFLOW = 7, SMX_CNT_SPECIMEN0 = 8 };

int smx_abi_version(void);
const char *smx_last_error(void);

/* device selection for the calling thread; returns the device count in *n_devices if non-NULL */
int smx_device_init(int device, int *n_devices);

int smx_panel_create(const smx_panel_desc *desc, smx_panel **out);
void smx_panel_destroy(smx_panel *panel);
size_t smx_counts_len(const smx_panel *panel);      /* SMX_CNT_SPECIMEN0 + n_specimens */
size_t smx_window_stride(const smx_panel *panel);   /* bytes per read in the window buffer: round16(2*search_len) */
size_t smx_hits_per_read(const smx_panel *panel);   /* 2 * n_primers */
size_t smx_bdist_per_read(const smx_panel *panel);  /* 2 * n_primers * max barcodes per primer */

/*
 * What smx_panel_create admits; anything else is SMX_ERR_UNSUPPORTED with the limit in the message:
 *   distinct primers 1..64, primer pairs 1..127, distinct barcodes 1..2048, barcodes on one primer 1..1024,
 *   primer length 1..64 with 0 <= k < length, barcode length 1..32 with 0 <= k_index < length,
 *   barcode_len_max + k_index <= 200, prefilter_min_len 0 or >= 2, search_len 1..256,
 *   and every tile plan the panel can launch (lean, slots, compact) within the LDS pool of a CU, 159744 bytes.  The last
 *   rule is what bounds large barcode lists in practice: the per-barcode ("slots") kernel keeps 64 bytes per distinct
 *   barcode of the panel, the count rounded up to a power of two.  Up to 1024 distinct barcodes that is 64 KiB; from
 *   1025 to 2048 it is 128 KiB and few panels still fit ("The admitted envelope"); above 2048 none can.  A
 *   panel with a plan over the pool is refused as a whole -- not accepted for the lean kernel and refused at the first
 *   --trim tails launch.
 *
 * smx_panel_plan: the launch plan smx_panel_create made, for inspection and tests.  Host only: no device is needed
 * or touched.  Per mode -- lean, slots (--trim tails where the lean kernel cannot report the extent, the d_bdist dump),
 * compact (panels with many primers; R = 0: the panel never launches it) -- the reads per tile, the dynamic LDS of one
 * workgroup, and the row (primer word bits, barcode scan variant, dense 0 / compact 1 / redo 2, default-flags
 * specialisation) of the kernel's instantiation list a launch gets: variant[1] with the primer prescan in front of it,
 * variant[0] without (a panel launches the one its pre_ok names; compact tiles exist with the prescan only, their variant[0]
 * is all zero).  With nitems > 0 every lean launch is a compact launch followed by a dense lean launch over the tiles
 * the compact one could not hold: that launch takes the lean tile and the rows redo[].  MBW .. CAPE are the tile layout's
 * sizes as the kernel computes them, SMX_TEST_CAPS applied.
 */
typedef struct smx_plan_variant { int32_t wbits, bsv, cm, sp; } smx_plan_variant;
typedef struct smx_plan_mode {
    int32_t R;                   /* reads per tile */
    uint32_t lds_bytes;          /* dynamic LDS of one workgroup */
    smx_plan_variant variant[2]; /* [0] launched without the prescan, [1] with it */
    int32_t MBW;                 /* tie-mask words per hit: ceil(max barcodes on one primer / 32) */
    int32_t G;                   /* barcode slots per hit: that maximum rounded up to a power of two */
    int32_t CAPH, CAPE;          /* hits and (hit, location) entries of one barcode round */
} smx_plan_mode;
typedef struct smx_plan_info {
    uint32_t lds_pool;           /* LDS a CU gives to workgroups: no lds_bytes above is larger */
    int32_t nitems;              /* records per compact tile; 0: no compact tiles */
    int32_t use64;               /* 64-bit primer words (a primer longer than 32 nt) */
    int32_t bs_ok;               /* bit-sliced barcode scan: one barcode length <= 16, k_index <= 7 */
    int32_t pre_ok, pre_tile;    /* primer prescan in front of every launch; it hands tile-major codes on */
    smx_plan_mode lean, slots, compact;
    smx_plan_variant redo[2];    /* the dense lean launch behind a compact one */
} smx_plan_info;
int smx_panel_plan(const smx_panel *panel, smx_plan_info *out);

/*
 * Cut the two end windows of each read (host, no device work): for read i with bases
 * bases[offsets[i] .. offsets[i+1]) and S' = min(search_len, len):
 *   windows[i*stride .. +S')            = first S' bases   (zero padded to search_len)
 *   windows[i*stride+search_len .. +S') = last  S' bases   (zero padded)
 * lens[i] = len.
 */
int smx_pack_windows(const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, int32_t search_len,
                     uint8_t *windows, int32_t *lens);

/*
 * The same two windows as 4-bit text codes (the transport format of the lanes: half the bytes across PCIe).  Code of a
 * base = its index in "ACGTNRYKMSWBDHV", 15 for anything else (such characters match no pattern character in either
 * format); per read: ceil(search_len / 2) bytes of head window, the same of tail window, base j in byte j / 2 (low nibble
 * first), unused nibbles 15; stride = smx_packed_stride(panel) = round16(2 * ceil(search_len / 2)).
 * *n_ascii_only (optional) counts the reads with a 'U' inside a window: the one letter the 4-bit alphabet cannot carry
 * faithfully (Bio.Seq complements U to A); a batch with any must be sent as ASCII windows.
 * smx_unpack_windows_device turns packed windows resident in device memory into the ASCII layout smx_batch_run_device takes.
 */
size_t smx_packed_stride(const smx_panel *panel);
int smx_pack_windows4(const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, int32_t search_len,
                      uint8_t *packed, int32_t *lens, uint32_t *n_ascii_only);
int smx_unpack_windows_device(const smx_panel *panel, void *stream, const uint8_t *d_packed, uint32_t n_reads,
                              uint8_t *d_windows);

/*
 * Run the hot path on windows already resident in device memory.  All pointers are DEVICE pointers;
 * `stream` is a hipStream_t (NULL = default stream).  Asynchronous: returns after enqueueing.
 *   d_ops          n_reads records
 *   d_extra        extra_cap records; d_n_extra one uint32, WRITTEN by the call (number of extra records produced,
 *                  may exceed extra_cap: then only the first extra_cap were stored); no need to clear it
 *   d_counts       smx_counts_len() uint64, accumulated into (not cleared)
 *   d_hits/d_bdist optional parity dumps (NULL to skip): n_reads*smx_hits_per_read() smx_hit and
 *                  n_reads*smx_bdist_per_read() int8 best distance per (read, primer, end, barcode slot), -1 none
 *                  d_bdist selects the per-barcode ("slots") kernel; d_hits alone is filled by whichever kernel the
 *                  panel's flags select (tail_end is then defined only under --trim tails)
 * Launches on one stream are ordered; a panel keeps one tile queue per stream it is launched on (at most 16
 * streams), so double-buffered callers may overlap launches of one panel on different streams.
 */
int smx_batch_run_device(const smx_panel *panel, void *stream, const uint8_t *d_windows, const int32_t *d_lens,
                         uint32_t n_reads, smx_op *d_ops, smx_op *d_extra, uint32_t extra_cap,
                         uint32_t *d_n_extra, uint64_t *d_counts, smx_hit *d_hits, int8_t *d_bdist);

/*
 * Tell the panel how many batches the caller keeps in flight on as many streams (default 1).  The demux kernel is a
 * persistent launch sized to the CUs' resident workgroup slots; with n batches in flight each launch takes 1/n of them, so
 * that kernels of different batches run side by side (the next batch's prescan beside this batch's demux kernel) instead
 * of queueing behind a launch that fills the machine.  Takes effect from the next launch; call it between batches.
 */
int smx_panel_set_streams(smx_panel *panel, int n_streams);

/*
 * Diagnostic: per-kernel device times of smx_batch_run_device on this panel.  enable != 0 makes every following launch
 * record HIP events around its kernels (transpose, primer DP, demux) on the launch stream; with ms != NULL the call waits
 * for the most recent instrumented launch and writes its three durations in milliseconds (0 for a kernel that did not
 * run; panels with many primers launch the demux kernel twice per batch -- compact tiles, then the reads of the tiles
 * that did not fit: the third duration covers both).  Off by default: the events cost a few microseconds per launch.
 */
int smx_debug_kernel_times(smx_panel *panel, int enable, float ms[3]);

/*
 * Convenience wrapper over host buffers: allocates device scratch, copies, runs, copies back, synchronises.
 * counts is accumulated into (host, smx_counts_len() uint64).  Returns SMX_ERR_OVERFLOW if extra_cap was too
 * small (n_extra then holds the required capacity) or a read exceeded the per-read operation limit.
 */
int smx_batch_run(const smx_panel *panel, const uint8_t *windows, const int32_t *lens, uint32_t n_reads,
                  smx_op *ops, smx_op *extra, uint32_t extra_cap, uint32_t *n_extra, uint64_t *counts,
                  smx_hit *hits, int8_t *bdist);

/*
 * Lanes: the asynchronous host-buffer path (pinned, double-buffered hand-off).  A lane owns a HIP
 * stream, page-locked host staging for one batch (windows + lengths in, records + counts out) and its device buffers.
 * Pipelines keep two or three lanes in flight: while lane A's kernels run, lane B's windows cross PCIe and lane C's
 * records are written out -- the replacement of the reference parent's pickled 1000-read batches
 * (io_utils.py:429-450, orchestration.py:447-456).
 *   smx_lane_create    max_reads = capacity of one batch
 *   smx_lane_windows / smx_lane_lens   pinned staging the packer fills (smx_pack_windows_batch writes there directly)
 *   smx_lane_submit    enqueue H2D copy, prescan + demux kernels, D2H copy on the lane's stream; returns at once
 *   smx_lane_submit_packed   the same for a staging filled with 4-bit windows (84 instead of 164 bytes per read at -l 80)
 *   smx_lane_wait      block until the lane's batch is done; *ops / *extra point into the lane's pinned result buffers
 *                      (valid until the next submit on this lane); counts (host, smx_counts_len() uint64) is accumulated
 *                      into.  SMX_ERR_OVERFLOW as for smx_batch_run (the extra buffer of a lane holds max_reads records).
 */
typedef struct smx_lane smx_lane;
int smx_lane_create(const smx_panel *panel, uint32_t max_reads, smx_lane **out);
void smx_lane_destroy(smx_lane *lane);
uint8_t *smx_lane_windows(smx_lane *lane);
int32_t *smx_lane_lens(smx_lane *lane);
int smx_lane_submit(smx_lane *lane, uint32_t n_reads);
/* the staging behind smx_lane_windows holds 4-bit windows (smx_pack_windows4_batch): H2D of half the bytes + unpack kernel */
int smx_lane_submit_packed(smx_lane *lane, uint32_t n_reads);
int smx_lane_wait(smx_lane *lane, const smx_op **ops, const smx_op **extra, uint32_t *n_extra, uint64_t *counts);

/*
 * One edlib-equivalent alignment on the device (Myers bit-vector kernel), for unit parity with the oracle.
 * mode 0 = HW (infix), 1 = SHW (prefix); IUPAC equalities always on; qlen <= 64.
 * *dist = -1 if the best distance exceeds k.  Up to cap (start,end) pairs are written, *nloc = true count.
 * Any k >= 0 (k >= qlen: every alignment is "within k") and any tlen >= 1; k < 0 gives *dist = -1.  In SHW mode no
 * optimal end lies beyond column qlen + min(k, qlen), and the device scans no further.
 * SMX_ERR_UNSUPPORTED for qlen outside 1..64, a query letter outside the IUPAC DNA alphabet, a mode other than 0 / 1 and
 * tlen < 1: refused by host code, before the device is asked.
 */
int smx_align(const char *query, int qlen, const char *target, int tlen, int k, int mode,
              int *dist, int *starts, int *ends, int cap, int *nloc);

/*
 * N alignments in one launch (trace level 3 and --color ask for thousands per batch; device workspace is cached).
 *   queries / qoff      n_queries distinct query strings (concatenated, n_queries + 1 offsets), each 1..64 letters
 *   targets / toff      n targets (concatenated, n + 1 offsets), each >= 1 letter
 *   qidx, k, mode       per alignment: query index, max distance 0..250 (k >= the query's length: every alignment is
 *                       "within k"), 0 = HW / 1 = SHW
 *   dist, nloc          per alignment: best distance (-1: above k) and number of optimal locations
 *   starts, ends        n x cap; the first min(nloc, cap) locations of alignment i at [i * cap ..); may be NULL if cap == 0
 * n == 0 is SMX_OK.  Otherwise, from host code before the device is asked: SMX_ERR_UNSUPPORTED for a query length outside
 * 1..64, a query letter outside the IUPAC DNA alphabet and an empty target; SMX_ERR_ARG for qidx >= n_queries, a mode above
 * 1 and k outside 0..250.
 */
int smx_align_batch(const char *queries, const uint32_t *qoff, uint32_t n_queries, const char *targets,
                    const uint64_t *toff, const uint32_t *qidx, const int32_t *k, const uint8_t *mode, uint32_t n,
                    int32_t *dist, int32_t *nloc, int32_t *starts, int32_t *ends, uint32_t cap);

/*
 * specimine: HW (infix) edit distances of long reads in batches -- query = a specimen's full read, target = one of its
 * partial reads (reference specimine.py:197-257, edlib.align(full, partial, mode="HW", k)).  Exact byte equality, no
 * IUPAC equalities.  Distance only.
 *   queries / qoff     n_queries queries (concatenated, n_queries + 1 offsets), each >= 1 byte; a query's Peq table,
 *                      (distinct bytes + 1) x ceil(len / 64) words, must fit the LDS (any DNA read up to ~250 kb)
 *   k                  per query: max distance, < 0 = none (-1 is returned for a distance above k)
 *   targets / toff     n_targets targets (concatenated, n_targets + 1 offsets), any length (empty: distance = query
 *                      length whatever k is, as edlib)
 *   jobs               each job pairs queries [q0, q0 + nq) with targets [t0, t0 + nt)
 * smx_mine_best_identity: per target of job j, at best[sum over earlier jobs of nt], the largest identity
 * = 1 - d / len(query) (IEEE double) over the job's queries with d != -1, identity >= min_identity and identity > 0;
 * 0 when there is none.  Each pair's identity goes straight into its target's best with a 64-bit atomic max, without a
 * distance matrix: device and host memory are bounded by the queries, the targets, sum(nq) and sum(nt); nothing grows
 * with sum(nq * nt).  Job target ranges may overlap (many jobs over one uploaded target set).
 * smx_mine_distances, kept for tests and inspection, writes job j's nq x nt distances row-major (one row per query) at
 * dist[sum over earlier jobs of nq * nt].
 * kernel_ms (may be NULL) receives the device time of the mining kernels (HIP events).
 */
typedef struct smx_mine_job {
    uint32_t q0, nq, t0, nt;
    double min_identity;      /* smx_mine_best_identity only */
} smx_mine_job;

int smx_mine_distances(const char *queries, const uint64_t *qoff, uint32_t n_queries, const int32_t *k, const char *targets,
                       const uint64_t *toff, uint32_t n_targets, const smx_mine_job *jobs, uint32_t n_jobs, int32_t *dist,
                       float *kernel_ms);
int smx_mine_best_identity(const char *queries, const uint64_t *qoff, uint32_t n_queries, const int32_t *k,
                           const char *targets, const uint64_t *toff, uint32_t n_targets, const smx_mine_job *jobs,
                           uint32_t n_jobs, double *best, float *kernel_ms);

/*
 * clusters: NW (global) edit distances of all pairs of reads within one specimen, in batches -- nothing in the reference
 * does this; edlib.align(a, b, mode="NW", k) is the definition.  Exact byte equality, no IUPAC
 * equalities.  Distance only.
 *   reads / roff       n_reads reads (concatenated, n_reads + 1 offsets), any length (an empty read is at distance
 *                      len(other) from any other); every read's Peq table must fit the LDS, as a specimine query's
 *   k                  per read: its max distance (< 0: no limit).  The limit of the pair (i, j) is max(k[i], k[j]), no
 *                      limit if either read has none: integers only, the device decides no pair in floating point
 *   jobs               each job is the reads [r0, r0 + n) of one specimen, its pairs the i < j among them.  Jobs of 0 or
 *                      1 reads are legal.  The ranges of two jobs may not overlap (SMX_ERR_ARG)
 * smx_pairs_neighbours: per job its symmetric adjacency bit matrix, n rows x ceil(n / 32) uint32 words, bit j of row i
 * (word j / 32, bit j % 32) set iff i != j and the pair's distance is within its limit; the diagonal and the bits >= n
 * are zero.  Job j's matrix follows the matrices of the earlier jobs (n = 1: one zero word, n = 0: nothing).  The kernel
 * writes whole words of the upper triangle (one wave ballot per 64 pairs), the library mirrors them: device and host
 * memory are bounded by the reads and sum(n * ceil(n / 32)) words; nothing is sized by n^2 integers.
 * smx_pairs_distances, kept for tests and inspection, writes job j's packed upper triangle, row-major over i < j (n (n - 1)
 * / 2 int32, -1 above the limit), after the triangles of the earlier jobs.
 * kernel_ms (may be NULL) receives the device time of the kernels (HIP events).
 */
typedef struct smx_pairs_job {
    uint32_t r0, n;
} smx_pairs_job;

int smx_pairs_distances(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k,
                        const smx_pairs_job *jobs, uint32_t n_jobs, int32_t *dist, float *kernel_ms);
int smx_pairs_neighbours(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k,
                         const smx_pairs_job *jobs, uint32_t n_jobs, uint32_t *adj, float *kernel_ms);

/*
 * consensus: every member read of a cluster aligned globally (NW) to the cluster's draft, with traceback, and the
 * alignments reduced to per-position votes -- nothing in the reference does this; it hands the step to an external
 * consensus tool.  Exact byte equality, as in clusters.
 *   reads / roff / k   as for smx_pairs_*.  The limit of a (draft, member) pair is max(k[draft], k[member]), no limit if
 *                      either has none.  A draft's Peq table must fit the LDS, as a read's in smx_pairs_*
 *   jobs               each job aligns the reads [r0, r0 + n) to the read `draft`, which may be one of them.  Jobs of
 *                      n = 0 are legal.  SMX_ERR_ARG, before anything is launched: an empty draft, an index out of range,
 *                      member ranges of two jobs that overlap
 * The pileup row of a member over a draft of m bases is m + 1 uint32 words.  Word p < m: bits 0-2 what the member has at
 * draft position p (0-3 = the bytes A C G T, 4 = any other byte, 5 = deletion), bits 3-10 the length of its insertion before
 * position p, clipped to 255, bits 11-22 the codes of the first SMX_CONS_MAX_INS inserted bytes, 3 bits each, in read
 * order.  Word m: bits 0-2 are 7, the rest is the insertion after the last base.  Of the optimal alignments the row is
 * the one the fixed walk from the end takes: diagonal if it is optimal, else up (deletion), else left (insertion).
 * smx_cons_pileup, kept for tests and inspection: job after job its n rows (n x (m + 1) words) and its n distances (-1
 * above the limit, and then a row of 0xFFFFFFFF).
 * smx_cons_votes, the production entry (the rows never leave the device): job after job its (m + 1) x
 * SMX_CONS_VOTE_WORDS table -- per position sym[6] (A, C, G, T, other, deletion), then ins[slot][code] for slot < 4 and
 * code < 5 (a member whose insertion before p has length L votes in slots 0 .. min(L, 4) - 1) -- over the members within
 * their limit, and aligned[j], the number of those.  No atomics: the table is the same from run to run.  n = 0: a zero table.
 * kernel_ms (may be NULL) receives the device time of the kernels (HIP events).
 */
#define SMX_CONS_MAX_INS 4
#define SMX_CONS_VOTE_WORDS (6 + 5 * SMX_CONS_MAX_INS)

typedef struct smx_cons_job {
    uint32_t draft, r0, n;   /* draft: an index into reads; members: reads [r0, r0 + n) */
} smx_cons_job;

int smx_cons_pileup(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k,
                    const smx_cons_job *jobs, uint32_t n_jobs, uint32_t *rows, int32_t *dist, float *kernel_ms);
int smx_cons_votes(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k,
                   const smx_cons_job *jobs, uint32_t n_jobs, uint32_t *votes, uint32_t *aligned, float *kernel_ms);

/*
 * variants: after the alignment and the vote of smx_cons_votes, in the same call and over the rows that are still on the
 * device, the columns of each job where a second allele has support, every member's allele at those columns, and how
 * the columns go together across the members -- nothing in the reference does this.
 *   reads .. n_jobs    as for smx_cons_votes; votes / aligned receive exactly what smx_cons_votes returns for them
 *   min_permille, min_reads   a candidate qualifies when n_minor >= min_reads and 1000 * n_minor >= min_permille * aligned[job]
 *   max_sites          1 .. SMX_CONS_MAX_SITES: the sites kept per job, and the first dimension of every table below
 * SMX_ERR_ARG, before anything is launched: max_sites of 0 or above SMX_CONS_MAX_SITES, min_permille above 1000.
 * Candidates, in the order (p, insertion before base) for the vote-table positions p = 0 .. m:
 *   kind 1, the insertion site before p: present = the votes of ins[0][0..4], absent = aligned - present; the minor allele
 *           is the smaller of the two, `present` on a tie; codes 1 = present, 0 = absent
 *   kind 0, the base site at p < m: over A, C, G, T and deletion (sym[0..3], sym[5]; sym[4] "other" is ignored) major = most
 *           votes, minor = second most, ties to the lower code in both; codes as in the row: 0-3 and 5
 * sites[job * max_sites + i], i < n_sites[job]: the first max_sites qualifying candidates; n_qualified[job]: how many
 * qualified.  Slots past n_sites are zero.
 * planes: job after job max_sites x 2 x ceil(n / 64) 64-bit words, plane[site][0 = minor | 1 = major][word]: bit i & 63 of
 * word i >> 6 is set when member i is within its limit and rows[i][pos] holds that allele (kind 1: `present` = the row's
 * insertion length is not zero).  A member with another symbol there, or above its limit, has neither bit.
 * link[((job * max_sites + s) * max_sites + t) * 4 ..], s < t < n_sites[job]: the members with (minor, minor), (minor at s,
 * major at t), (major at s, minor at t), (major, major); every other entry is zero.
 * No atomics: every table is the same from run to run.  A job of n = 0 has zero tables and n_sites = n_qualified = 0.
 */
#define SMX_CONS_MAX_SITES 64

typedef struct smx_cons_site {
    uint32_t pos;                 /* the vote-table position p */
    uint8_t kind, major, minor, pad;
    uint32_t n_major, n_minor;
} smx_cons_site;

int smx_cons_phase(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k,
                   const smx_cons_job *jobs, uint32_t n_jobs, uint32_t min_permille, uint32_t min_reads, uint32_t max_sites,
                   uint32_t *votes, uint32_t *aligned, smx_cons_site *sites, uint32_t *n_sites, uint32_t *n_qualified,
                   uint64_t *planes, uint32_t *link, float *kernel_ms);

/*
 * support: after the alignment and the vote of smx_cons_votes, in the same call and over the rows that are still on the
 * device, the vote taken again over SMX_CONS_REPLICATES subsets of each job's members at once, for up to
 * SMX_CONS_MAX_LEVELS sets of subsets (levels): which subsets would call each column as the draft has it (DESIGN.md
 * section 20) -- nothing in the reference does this.
 *   reads .. n_jobs    as for smx_cons_votes; votes / aligned receive exactly what smx_cons_votes returns for them
 *   masks              n_levels x (the sum of the jobs' n) 64-bit words: level after level, within a level job after job in
 *                      the order given, one word per member.  Replicate b (0..63) of a level is the set of members whose
 *                      word has bit b set; its voters are those of them within their limit
 * SMX_ERR_ARG, before the device is asked for and also where n_jobs is 0: n_levels of 0 or above SMX_CONS_MAX_LEVELS, a null
 * masks while some job has members.
 * Over the voters of replicate b at column p of a draft of m bases: a[0..3] the row words with symbol A, C, G, T, del those
 * with symbol 5, ins those with an insertion before p, n_b the voters.  With dc the code of the draft's byte at p (0-3, 4 =
 * any other byte), replicate b keeps column p iff
 *     !(2 ins > n_b)  &&  ( p == m  ||  ( !(2 del > n_b)  &&  ( max a == 0  ||  (dc < 4 && a[dc] == max a) ) ) )
 * agree: job after job, level after level, m + 1 words: bit b of word p is set iff replicate b keeps column p.
 * sub_aligned[(job * n_levels + level) * 64 + b]: n_b.  A replicate without voters keeps every column: the caller decides
 * what that means.  A job of n = 0 has all-ones words and zero counts.  No atomics: the same from run to run.
 */
#define SMX_CONS_REPLICATES 64
#define SMX_CONS_MAX_LEVELS 16

int smx_cons_resample(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k,
                      const smx_cons_job *jobs, uint32_t n_jobs, const uint64_t *masks, uint32_t n_levels,
                      uint32_t *votes, uint32_t *aligned, uint64_t *agree, uint32_t *sub_aligned, float *kernel_ms);

/*
 * errors: after the alignment and the vote of smx_cons_votes, in the same call and over the rows that are still on the
 * device, every member's row reduced against its job's draft and the read's quality bytes to the error profile of the
 * reads -- nothing in the reference does this.
 *   reads .. n_jobs    as for smx_cons_votes; votes / aligned receive exactly what smx_cons_votes returns for them
 *   quals              the FASTQ quality bytes as they stand in the file, in the layout of reads (the same roff).  The
 *                      draft's own quality bytes are never read
 * SMX_ERR_ARG, before the device is asked for: a null quals, per_member or tables while some job has members.
 * With dc the code of the draft's byte at column p < m (0-3, 4 = any other byte) and, of the member's row word p, sym = bits
 * 0-2 and L = bits 3-10, a column is a match (sym <= 3, dc <= 3, sym == dc), a sub (sym <= 3, dc <= 3, sym != dc), a del
 * (sym == 5) or other (sym == 4 or dc == 4); L > 0 at p <= m is one insertion event of L bases.  The column's base is read
 * byte rp(p) = sum over q < p of ((sym_q <= 4) + L_q) + L_p, the bases inserted before it are the L_p bytes before that:
 * exact unless some L is 255, the clipped value; such a member is `clipped`.
 * per_member: job after job, member after member, SMX_PROFILE_MEMBER_WORDS words: match, sub, del, other, ins_events,
 * ins_bases (the sum of L as stored), clipped (0 / 1), 0.  A member above its limit has eight zeros.
 * tables: job after job SMX_PROFILE_JOB_WORDS words, summed over the members within their limit:
 *   q[64][3]      per Phred bin (byte b: b < 33 ? 0 : min(b - 33, 63)) the read bases in a match column, in a sub or other
 *                 column, and the inserted bases (all L of them, each under its own byte's bin).  Unclipped members only
 *   subst[4][5]   dc (0-3) x the member's symbol: 0-3 = A C G T, 4 = deletion
 *   ins[6]        the kept inserted codes 0-4 (the first SMX_CONS_MAX_INS of an insertion), then the bases beyond those
 *   hp[8][7]      per run of the draft -- a maximal stretch [s, s + r) of one code b <= 3 -- and member: length class
 *                 min(r, 8) - 1 x (delta + 3), delta = clamp(obs - r, -3, +3), obs = the run's columns where sym == b plus
 *                 the kept inserted codes equal to b before the columns s .. s + r
 * Integer adds only: every word is the same from run to run.  A job of n = 0, or without a member within its limit, has
 * zero tables.
 */
#define SMX_PROFILE_MEMBER_WORDS 8
#define SMX_PROFILE_Q_BINS 64
#define SMX_PROFILE_JOB_WORDS (SMX_PROFILE_Q_BINS * 3 + 4 * 5 + 6 + 8 * 7)

int smx_cons_profile(const char *reads, const uint64_t *roff, uint32_t n_reads, const int32_t *k,
                     const smx_cons_job *jobs, uint32_t n_jobs, const unsigned char *quals, uint32_t *votes,
                     uint32_t *aligned, uint32_t *per_member, uint32_t *tables, float *kernel_ms);

/*
 * crosstalk: NW (global) edit distances of every read of a run to every consensus (ref) of the run, reduced on the device
 * to each read's nearest ref of its own group and its nearest ref of any other group -- nothing in the reference does
 * this.  The pair code is clusters': exact byte equality, distance only.
 *   seqs / off         n_seqs sequences (concatenated, n_seqs + 1 offsets): the reads and the refs share one array, as
 *                      the drafts and members of smx_cons_* do.  A read may have any length (an empty read is at distance
 *                      len(ref) from a ref); a ref is not empty and its Peq table must fit the LDS, as a read's in
 *                      smx_pairs_* (SMX_ERR_UNSUPPORTED)
 *   k                  per sequence: its max distance (< 0: no limit).  The limit of a (ref, read) pair is
 *                      max(k[ref], k[read]), no limit if either has none: the smx_pairs_* rule
 *   group              per sequence: a ref is "own" to a read iff their groups are equal
 *   jobs               each job compares the refs [q0, q0 + nq) with the reads [t0, t0 + nt).  nq = 0 and nt = 0 are
 *                      legal.  Ref ranges of different jobs may overlap (many jobs over one ref set).  SMX_ERR_ARG, before
 *                      anything is launched: an empty ref, an index out of range, read ranges of two jobs that overlap
 * smx_nearest: job after job, nt entries of best_own and of best_other: ((uint64_t)d << 32) | ref for the ref (its index
 * in seqs) at the smallest distance d within the pair's limit among the job's refs of the read's group (best_own) and
 * among all its other refs (best_other); of refs at equal distance the lowest index; UINT64_MAX where there is none.
 * The device keeps one 64-bit minimum per read and array (atomicMin over a total order): the arrays are the same from
 * run to run, and device and host memory are bounded by the sequences and sum(nt) -- nothing is sized by sum(nq * nt).
 * SMX_NEAREST_MIN_CHUNKS (environment) overrides the number of chunks the plan keeps the call above when it chooses how
 * many refs a workgroup takes in a row; it changes the speed, never the result.
 * smx_nearest_distances, kept for tests and inspection, writes job after job its nq x nt distances, one row per ref
 * (int32, -1 above the limit).
 * kernel_ms (may be NULL) receives the device time of the kernels (HIP events).
 */
typedef struct smx_nearest_job {
    uint32_t q0, nq, t0, nt;   /* refs [q0, q0 + nq), reads [t0, t0 + nt): indices into seqs */
} smx_nearest_job;

int smx_nearest(const char *seqs, const uint64_t *off, uint32_t n_seqs, const int32_t *k, const uint32_t *group,
                const smx_nearest_job *jobs, uint32_t n_jobs, uint64_t *best_own, uint64_t *best_other, float *kernel_ms);
int smx_nearest_distances(const char *seqs, const uint64_t *off, uint32_t n_seqs, const int32_t *k, const uint32_t *group,
                          const smx_nearest_job *jobs, uint32_t n_jobs, int32_t *dist, float *kernel_ms);

/*
 * identify: the best few records of a reference FASTA for every consensus sequence of a run -- nothing in the reference
 * does this.  The pair code is specimine's (HW, infix edit distance, exact byte equality).
 *   seqs / off         n_seqs sequences (concatenated, n_seqs + 1 offsets): queries and targets share one array.  No
 *                      query or target may be empty (SMX_ERR_ARG)
 *   k                  per sequence: its max distance (< 0: no limit).  The limit of a pair is its pattern's
 *   jobs               each job compares the queries [q0, q0 + nq) with the targets [t0, t0 + nt).  nq = 0 and nt = 0 are
 *                      legal.  Target ranges of different jobs may overlap (many jobs over one uploaded database); query
 *                      ranges may not (SMX_ERR_ARG: every query has one output row).  nt <= 2^24 (SMX_ERR_UNSUPPORTED)
 *   K                  hits kept per query, 1..SMX_HITS_MAX_K (SMX_ERR_ARG)
 *   min_cov_permille   0..1000 (SMX_ERR_ARG)
 * The pair rule: of a (query, target) pair the shorter sequence is the pattern, the other the text, the query at equal
 * length; d = HW(pattern in text) within k[pattern], and the pair counts only if
 * len(pattern) * 1000 >= min_cov_permille * len(text).  A pattern must be shorter than 2^19 bytes and its Peq table must
 * fit the LDS (SMX_ERR_UNSUPPORTED).  Every refusal comes before anything is launched.
 * smx_best_hits: job after job, per query K keys in ascending order, padded with UINT64_MAX:
 *   bits 63-43  ((uint64_t)d << 20) / len(pattern), integer division
 *   bits 42-24  d
 *   bits 23-0   the target's index within the job, t - t0
 * so that unsigned order is "lower edit fraction, then fewer edits, then lower target index".  The device keeps K 64-bit
 * slots per query and inserts with atomicMin over this total order: the keys are the same from run to run, and device
 * and host memory are bounded by the sequences and sum(nq) * K -- nothing is sized by sum(nq * nt).
 * smx_best_hits_distances, kept for tests and inspection, writes job after job its nq x nt distances, one row per query
 * (int32; -1 above the limit and for pairs that coverage excludes).
 * kernel_ms (may be NULL) receives the device time of the kernels (HIP events).
 */
#define SMX_HITS_MAX_K 16

typedef struct smx_hits_job {
    uint32_t q0, nq, t0, nt;   /* queries [q0, q0 + nq), targets [t0, t0 + nt): indices into seqs */
} smx_hits_job;

int smx_best_hits(const char *seqs, const uint64_t *off, uint32_t n_seqs, const int32_t *k, const smx_hits_job *jobs,
                  uint32_t n_jobs, uint32_t K, uint32_t min_cov_permille, uint64_t *keys, float *kernel_ms);
int smx_best_hits_distances(const char *seqs, const uint64_t *off, uint32_t n_seqs, const int32_t *k,
                            const smx_hits_job *jobs, uint32_t n_jobs, uint32_t K, uint32_t min_cov_permille, int32_t *dist,
                            float *kernel_ms);

/*
 * bimera: how far a prefix (and a suffix) of every called sequence of a run lies within e edits of every candidate
 * parent, for every e in 0..E -- what a PCR chimera check needs; nothing in the reference does this (DESIGN.md section
 * 19).  D(i, j) is the unit-cost edit distance (exact byte equality) of q[0:i] and r[0:j], anchored at both starts, and
 *   reach(q, r, e)    the largest i in 0..len(q) with min over j of D(i, j) <= e: the longest prefix of q within e edits
 *                     of some prefix of r; non-decreasing in e
 *   reach_r(q, r, e)  reach(reversed q, reversed r, e): the same for suffixes
 * computed exactly by furthest-reaching diagonals (HIP kernel smx_reach.hip), not by a bit-vector scan.
 *   seqs / off         n_seqs sequences (concatenated, n_seqs + 1 offsets): queries and targets share one array.  No
 *                      query or target may be empty (SMX_ERR_ARG); none longer than 2^30 - 1 (SMX_ERR_UNSUPPORTED)
 *   weight / need      per sequence.  Target t counts for query q iff t != q (index in seqs) and weight[t] >= need[q]
 *   jobs               each job compares the queries [q0, q0 + nq) with the targets [t0, t0 + nt).  nq = 0 and nt = 0 are
 *                      legal.  Target ranges of different jobs may overlap; query ranges may not (SMX_ERR_ARG: every
 *                      query has one output row)
 *   E                  0..SMX_REACH_MAX_E (SMX_ERR_ARG)
 * Every refusal comes before anything is launched.
 * smx_prefix_reach: job after job, per query, per side (0 = prefix / left, 1 = suffix / right), per e in 0..E, 2 keys in
 * ascending order, padded with UINT64_MAX:
 *   bits 63-32  0xFFFFFFFF - reach
 *   bits 31-0   t, the target's index in seqs
 * so that unsigned order is "longer reach, then lower index".  Every eligible target is offered at every e.  The device
 * keeps the slots and inserts with atomicMin over this total order: the keys are the same from run to run, and device
 * and host memory are bounded by the sequences and sum(nq) * 4 (E + 1) keys -- nothing is sized by sum(nq * nt).  The
 * top two of a union are the top two of its pieces' top twos, so calls over pieces of a parent pool merge exactly.
 * smx_prefix_reach_matrix, kept for tests and inspection, writes job after job its nq x nt x 2 x (E + 1) values (query,
 * target, side, e), UINT32_MAX where the target is not eligible.
 * kernel_ms (may be NULL) receives the device time of the kernel (HIP events).
 */
#define SMX_REACH_MAX_E 15

typedef struct smx_reach_job {
    uint32_t q0, nq, t0, nt;   /* queries [q0, q0 + nq), targets [t0, t0 + nt): indices into seqs */
} smx_reach_job;

int smx_prefix_reach(const char *seqs, const uint64_t *off, uint32_t n_seqs, const uint32_t *weight, const uint32_t *need,
                     const smx_reach_job *jobs, uint32_t n_jobs, uint32_t E, uint64_t *keys, float *kernel_ms);
int smx_prefix_reach_matrix(const char *seqs, const uint64_t *off, uint32_t n_seqs, const uint32_t *weight,
                            const uint32_t *need, const smx_reach_job *jobs, uint32_t n_jobs, uint32_t E, uint32_t *reach,
                            float *kernel_ms);

/*
 * tree: the neighbour-joining tree of n tips from their integer distances -- the join that specimux-tree builds over
 * the called sequences of a run; nothing in the reference does this.  The hot path is double
 * arithmetic, and the algorithm is fixed to the last operation (smx_nj_core.h: the order of every operation, no fused
 * multiply-add, ties by the smallest slots), so the records are the same bits from run to run and equal to the ones a
 * host loop over the same functions computes.
 *   tri                the packed upper triangle, row-major over i < j, n (n - 1) / 2 int32: the layout
 *                      smx_pairs_distances writes.  Every entry is >= 0 (SMX_ERR_ARG)
 *   n                  0..SMX_NJ_MAX_N tips (SMX_ERR_UNSUPPORTED above: the device keeps n x n doubles, 2 GiB at the most)
 *   merges             max(n - 3, 0) records.  Tips are the nodes 0..n-1; merge t joins the nodes a and b (the smaller
 *                      slot's first) into the node n + t.  n_active is the number of live nodes before the merge, d their
 *                      distance and ra, rb their row sums then: the branch lengths follow on the host,
 *                      la = d / 2 + (ra - rb) / (2 (n_active - 2)), lb = d - la
 *   last / last_d      the three nodes that remain and their distances d01, d02, d12.  n <= 3 launches nothing: last is
 *                      0..n-1 and last_d the given distances, the entries without a node or a pair zeroed
 * Every refusal comes before anything is launched.  kernel_ms (may be NULL) receives the device time of the kernels
 * (HIP events).
 */
#define SMX_NJ_MAX_N 16384

typedef struct smx_nj_merge {
    uint32_t a, b, n_active, pad;   /* pad = 0 */
    double d, ra, rb;
} smx_nj_merge;

int smx_nj(const int32_t *tri, uint32_t n, smx_nj_merge *merges, uint32_t last[3], double last_d[3], float *kernel_ms);

/*
 * msa: the progressive multiple alignment of n sequences along a guide tree -- what specimux-msa writes; nothing in the
 * reference does this.  Every merge of the tree aligns the profiles of its two children by an
 * integer-weighted dynamic programme with traceback; everything is integer and fixed to the last tie-break
 * (smx_msa_core.h), so the rows, lengths and costs are the same bytes from run to run and equal to a host loop's.
 *   seqs, off          n sequences back to back, n + 1 offsets; none is empty (SMX_ERR_ARG) or longer than
 *                      SMX_MSA_MAX_COLS (SMX_ERR_UNSUPPORTED).  A C G T (upper case) are four symbols, every other byte
 *                      is a fifth one that equals itself
 *   n                  0..SMX_MSA_MAX_N (SMX_ERR_UNSUPPORTED above)
 *   merges             n - 1 records: merge t joins the nodes a != b, both < n + t, into the node n + t; the tips are the
 *                      nodes 0..n-1 and every node is a child at most once (SMX_ERR_ARG otherwise)
 *   mismatch, gap      the weights X and G, 1..1000 each (SMX_ERR_ARG)
 *   cap_cols           the columns a row of `rows` has room for
 *   rows               n x cap_cols bytes; receives n rows of stride *n_cols: tip i's bytes at its columns, '-' elsewhere
 *   n_cols             the columns of the alignment.  If it exceeds cap_cols the call returns SMX_ERR_OVERFLOW with
 *                      *n_cols set, lens and costs filled and rows untouched: call again with that many
 *   lens, costs        n - 1 entries: the columns of node n + t, and the cost of merge t -- the sum over the tips x under
 *                      a and y under b of the pairwise cost of their rows (both gaps 0, one gap G, different symbols X)
 * A node of more than SMX_MSA_MAX_COLS columns ends the call with SMX_ERR_UNSUPPORTED.  Every other refusal comes before
 * anything is launched.  n = 0 writes nothing but *n_cols = 0; n = 1 returns the sequence.  kernel_ms (may be NULL)
 * receives the device time of the kernels (HIP events), level after level.
 */
#define SMX_MSA_MAX_N    4096
#define SMX_MSA_MAX_COLS 8192

typedef struct smx_msa_merge { uint32_t a, b; } smx_msa_merge;

int smx_msa(const char *seqs, const uint64_t *off, uint32_t n, const smx_msa_merge *merges, uint32_t mismatch, uint32_t gap,
            uint32_t cap_cols, uint8_t *rows, uint32_t *n_cols, uint32_t *lens, uint64_t *costs, float *kernel_ms);

/*
 * Diagnostic (tools/msa_bench.py): where the last smx_msa call of this process that asked for kernel_ms spent its device
 * time.  level_ms receives the time of the tree's levels in order, min(*n_levels, cap_levels) of them; tips_rows_ms the
 * time of the tips launch and of the rows launch; phase_us the time of the merge kernel's three phases (forward, walk
 * back, build), summed over the call's merges as thread 0 of each workgroup saw it on the device's wall clock -- zeros
 * unless the call ran with SMX_MSA_PHASE_TIMING set in the environment.
 */
int smx_msa_debug_times(float *level_ms, uint32_t cap_levels, uint32_t *n_levels, float tips_rows_ms[2], double phase_us[3]);

/*
 * Match statistics (specimux-stats; reference trace_stats.py): the "pool -> primer pair -> outcome" tables counted on the
 * device from what smx_batch_run_device leaves there -- the lean hit dump (d_hits without d_bdist) and the primary
 * records -- instead of from a trace TSV.  Every row the reference's tool would build from a read's trace events (one
 * per candidate match, or one synthesised row for a read without any) is packed into a 64-bit key and counted in an
 * open-addressing hash table of (key, 64-bit count) in device memory that lives for the whole run.
 *
 * Key layout (bit 0 = least significant; names come back on the host from the panel):
 *   [0, 2)    orientation: 0 unknown, 1 forward, 2 reverse
 *   [2, 14)   1 + index of the attempted primer pair (pair_fwd / pair_rev / pair_pool order); 0 = the read has no
 *             candidate (or was dropped by the length filter): every other field below is then 0 except `first`
 *   14        forward primer matched          15        reverse primer matched
 *   [16, 29)  1 + global index of the forward barcode (first of the tied best), 0 = none
 *   [29, 42)  the same for the reverse barcode
 *   [42, 45)  SMX_STATS_CLASS_*: the read-level resolution shared by the surviving candidates, or DISCARDED
 *   45        first candidate of its read (the rows `--count-by sequences` counts)
 * ~0 marks an empty slot.  Limits: n_pairs <= 4094, n_barcodes <= 8190 (smx_stats_create checks).
 *
 *   smx_stats_create            capacity = number of slots, rounded up to a power of two (>= 8)
 *   smx_stats_accumulate_device asynchronous, ordered on `stream` behind the batch that produced d_hits / d_ops (both
 *                               DEVICE pointers, n_reads * smx_hits_per_read() hits and n_reads records).  Reads whose
 *                               primary record carries SMX_OPF_TRIM_EMPTY cannot be decided from the record; their
 *                               indices go to d_fallback (fallback_cap uint32; may be NULL with cap 0) and
 *                               *d_n_fallback (one uint32, WRITTEN by the call; may exceed fallback_cap, then only the
 *                               first fallback_cap were stored) and they add nothing to the table: the host adds their rows.
 *   smx_stats_read              waits for the device, then copies the occupied slots out (any order).  *n = number of
 *                               distinct keys; SMX_ERR_ARG when cap < *n.  If any increment found the table full, the
 *                               call fails with SMX_ERR_OVERFLOW, *dropped = the lost increments, and nothing is copied.
 *   smx_stats_clear             empty the table (asynchronous on `stream`)
 */
enum { SMX_STATS_CLASS_UNKNOWN = 0, SMX_STATS_CLASS_FULL = 1, SMX_STATS_CLASS_PARTIAL_FWD = 2,
       SMX_STATS_CLASS_PARTIAL_REV = 3, SMX_STATS_CLASS_MULTIPLE = 4, SMX_STATS_CLASS_DISCARDED = 5 };
#define SMX_STATS_PAIR_SHIFT 2
#define SMX_STATS_P1_SHIFT 14
#define SMX_STATS_P2_SHIFT 15
#define SMX_STATS_B1_SHIFT 16
#define SMX_STATS_B2_SHIFT 29
#define SMX_STATS_CLASS_SHIFT 42
#define SMX_STATS_FIRST_SHIFT 45

typedef struct smx_stats smx_stats;
int smx_stats_create(const smx_panel *panel, uint32_t capacity, smx_stats **out);
void smx_stats_destroy(smx_stats *stats);
int smx_stats_accumulate_device(smx_stats *stats, void *stream, const smx_hit *d_hits, const smx_op *d_ops,
                                uint32_t n_reads, uint32_t *d_fallback, uint32_t fallback_cap, uint32_t *d_n_fallback);
int smx_stats_read(smx_stats *stats, uint64_t *keys, uint64_t *counts, uint32_t cap, uint32_t *n, uint64_t *dropped);
int smx_stats_clear(smx_stats *stats, void *stream);

/*
 * Lanes that count: a lane with a statistics table attached leaves the rows of every batch in that table, in the same
 * pass that produces the batch's records (an ordinary `-F` run then has its stats table as a by-product).
 *   smx_lane_attach_stats   stats = NULL detaches.  SMX_ERR_ARG if `stats` was created on another panel or the lane holds a
 *                           batch in flight.  The first attach allocates, for the life of the lane, a device buffer of
 *                           max_reads * smx_hits_per_read() smx_hit and a 1 + max_reads uint32 fallback list (device, and
 *                           a pinned copy); a lane that was never attached allocates nothing and enqueues exactly what
 *                           it did before.  Attaching waits for the device, so a smx_stats_clear enqueued earlier on any
 *                           stream is complete before the lane's first batch.  The table must outlive the attachment.
 *   smx_lane_submit[_packed] with a table attached: the demux launch also gets the lane's hit buffer (no d_bdist: the
 *                           panel's own kernel variant runs), smx_stats_accumulate_device follows on the lane's stream over
 *                           the lane's records and hits, then the fallback count and indices are copied to the pinned list.
 *                           Several lanes may count into one table at a time.
 *   smx_lane_fallback       after smx_lane_wait, until the next submit on that lane: the batch's reads the device could
 *                           not decide (smx_stats_accumulate_device's fallback list; any order), *idx pointing into the
 *                           lane's pinned list.  Also valid when smx_lane_wait returned SMX_ERR_OVERFLOW: the rows of such
 *                           a batch ARE in the table (counting needs the primary records only), so a caller that runs the
 *                           batch again for its records must not count it again.  SMX_ERR_ARG if the retired batch was
 *                           submitted without a table.
 */
int smx_lane_attach_stats(smx_lane *lane, smx_stats *stats);
int smx_lane_fallback(smx_lane *lane, const uint32_t **idx, uint32_t *n);

/*
 * RCCL reduction of the per-specimen counts over xGMI (one communicator per process/GPU).
 * smx_comm_unique_id fills a 128-byte id on rank 0; broadcast it by any means, then every rank calls
 * smx_comm_init.  smx_counts_allreduce sums d_counts (device pointer) in place across ranks.
 */
int smx_comm_unique_id(uint8_t id[128]);
int smx_comm_init(const uint8_t id[128], int n_ranks, int rank, void **comm_out);
int smx_counts_allreduce(uint64_t *d_counts, size_t n, void *comm, void *stream);
void smx_comm_destroy(void *comm);


/* ------------------------------------------------------------------------------------------------
 * Host streaming helpers: the steps on either side of the hot path.
 *
 *   smx_reader_*            <- open_sequence_file / SeqIO.parse + iter_batches
 *                              (src/specimux/io_utils.py:380-450, orchestration.py:447-456): FASTQ / FASTA,
 *                              plain or gzip; id = first whitespace-delimited word of the title; wrapped
 *                              sequence / quality lines accepted (Biopython FastqGeneralIterator rules)
 *   smx_pack_windows_batch  <- the end slices of match_one_end, straight from a parsed batch
 *   smx_writer_*            <- create_write_operation's slicing + OutputManager.write_sequence
 *                              (demultiplex.py:74-78, io_utils.py:197-268): orientation, trim, header
 *                              "{id} {p1d,b1d,b2d,p2d} pool={pool} primers={p1}+{p2} {sample}", path
 *                              {full|partial|unknown}/{pool}/{p1}-{p2}/{prefix}{sample}.{fastq|fasta} and the
 *                              pool-level copy of full matches.  Append-only, buffered per file.
 * Pure host code (no device work); a batch owns its memory, so reading batch i+1 may overlap the GPU run
 * of batch i and the writing of batch i-1 from different threads.
 */
typedef struct smx_reader smx_reader;
typedef struct smx_batch smx_batch;
typedef struct smx_writer smx_writer;

int smx_reader_open(const char *path, smx_reader **out, int *is_fastq);
/* the records that START inside bytes [lo, hi) of an uncompressed 4-line FASTQ (multi-GPU sharding of one file: the
 * ranges of all ranks partition the records); SMX_ERR_UNSUPPORTED for compressed, FASTA or irregular input */
int smx_reader_open_range(const char *path, uint64_t lo, uint64_t hi, smx_reader **out, int *is_fastq);
void smx_reader_close(smx_reader *reader);
smx_batch *smx_batch_new(void);
void smx_batch_free(smx_batch *batch);
/* parse up to max_reads records (and at most ~max_bytes of sequence data, 0 = no limit) into `batch`;
 * *n_read = 0 at end of file */
int smx_reader_next(smx_reader *reader, uint32_t max_reads, uint64_t max_bytes, smx_batch *batch, uint32_t *n_read);
uint32_t smx_batch_size(const smx_batch *batch);
/* record i: pointers into the batch (valid until the batch is refilled or freed); qual == NULL for FASTA */
int smx_batch_record(const smx_batch *batch, uint32_t i, const char **id, uint32_t *id_len, const char **seq,
                     const char **qual, uint32_t *seq_len);
/* record i's whole title: the header line after '@' / '>' (and any white space behind it), trailing white space
 * stripped; its first white-space-delimited word is the id smx_batch_record gives */
int smx_batch_title(const smx_batch *batch, uint32_t i, const char **title, uint32_t *title_len);
/* append every record of the batch, untrimmed, to one of two files: record i goes to flagged_path if flags[i] != 0, else to
 * clean_path (either may be NULL: those records are dropped).  "@title\nseq\n+\nqual\n", or ">title\nseq\n" for FASTA
 * records.  The files are opened for appending and closed again; the caller truncates them before the first batch. */
int smx_batch_write_split(const smx_batch *batch, const uint8_t *flags, const char *clean_path, const char *flagged_path);
int smx_pack_windows_batch(const smx_batch *batch, int32_t search_len, uint8_t *windows, int32_t *lens);
int smx_pack_windows4_batch(const smx_batch *batch, int32_t search_len, uint8_t *packed, int32_t *lens, uint32_t *n_ascii_only);

/* index -> name tables for the record headers and paths: concatenated strings with n+1 offsets each */
typedef struct smx_names {
    const char *specimens; const uint32_t *specimen_off; uint32_t n_specimens;
    const char *pools;     const uint32_t *pool_off;     uint32_t n_pools;
    const char *primers;   const uint32_t *primer_off;   uint32_t n_primers;
    const char *barcodes;  const uint32_t *barcode_off;  uint32_t n_barcodes;
} smx_names;

int smx_writer_open(const char *output_dir, const char *prefix, int is_fastq, const smx_names *names,
                    smx_writer **out);
/* format and append every write operation of the batch: ops[n_reads] primary records + extra[n_extra] */
int smx_writer_write(smx_writer *writer, const smx_batch *batch, const smx_op *ops, uint32_t n_reads,
                     const smx_op *extra, uint32_t n_extra);
int smx_writer_close(smx_writer *writer);   /* flushes; returns the first I/O error seen, if any */

/*
 * Inner scan (specimux-chimera): every pattern against the WHOLE read, reporting where it matches outside the two end
 * windows the demultiplexer searches.  Stand-alone, no panel handle.  Exact, IUPAC equalities as in the demux kernels (a
 * read byte outside the 15 upper-case letters matches nothing).
 *   patterns / poff   n_patterns (1..128) patterns (concatenated, n_patterns + 1 offsets), each 1..64 IUPAC letters
 *   k                 per pattern: threshold, 0 <= k < length
 *   bases / off       n_reads reads (concatenated, n_reads + 1 offsets), any length, empty allowed
 *   margin            columns margin <= c < len - margin of a read are internal (margin >= 0)
 *   max_hits          H, 1..8
 * D(c) = the last row of the HW (infix) DP of the pattern against the whole read at 0-based column c, i.e. the best NW
 * distance of the pattern to a read substring that ends at c.  A hit is a maximal run of consecutive internal columns with
 * D(c) <= k; its distance is the minimum of D over the run, its end the first column of the run with that minimum.
 *   nhit[r * Q + j]                      number of hits of pattern j in read r, saturating at 255
 *   hit_dist / hit_end [(r * Q + j) * H + h]   the first min(nhit, H) hits in column order; unused slots -1 / 0
 * budget_bytes (0 = 1 GiB) bounds the device memory of one launch group: larger inputs run as several chunks of whole
 * reads inside the call (a single read larger than the budget still runs, alone).  kernel_ms (may be NULL) receives
 * the device time of the kernels (HIP events).  smx_inner_scan_batch reads the records of a reader batch in place.
 */
int smx_inner_scan(const char *patterns, const uint32_t *poff, uint32_t n_patterns, const int32_t *k, const uint8_t *bases,
                   const uint64_t *off, uint32_t n_reads, int32_t margin, uint32_t max_hits, uint64_t budget_bytes,
                   uint8_t *nhit, int8_t *hit_dist, int32_t *hit_end, float *kernel_ms);
int smx_inner_scan_batch(const smx_batch *batch, const char *patterns, const uint32_t *poff, uint32_t n_patterns,
                         const int32_t *k, int32_t margin, uint32_t max_hits, uint64_t budget_bytes, uint8_t *nhit,
                         int8_t *hit_dist, int32_t *hit_end, float *kernel_ms);

/*
 * Barcode survey (specimux-barcodes): which sequences sit on the reads where a barcode should be, next to a primer that was
 * recognised -- counted on the device from what smx_batch_run_device was given and left there (the ASCII windows, the
 * lengths, the hit dump), then explained by candidate barcodes.  With S = search_len, Lb = barcode_len_max, k = k_index and
 * W = Lb + k; smx_flank_create refuses (SMX_ERR_UNSUPPORTED) W > SMX_FLANK_MAX_W and panels whose barcodes are not all
 * Lb long.
 *
 * Flank of a hit h = hits[i][2 * p + e] with h.pdist >= 0 (end e: 0 = A, 1 = B, as in smx_hit).  The end string's stored
 * window is the tail window for B and the reverse complement of the head window for A (window position j = complement of
 * head[S - 1 - j]); only reads with lens[i] >= S are taken, and for them reference coordinate c is window position
 * c - (lens[i] - S).  The flank is the flen = min(W, S - 1 - j_end) bases behind j_end = h.first_end - (lens[i] - S): the
 * prefix of the string the demultiplexer searches for barcode_rc (SHW from first_end + 1).  It lies inside the window,
 * because the window ends where the string ends.
 *
 * Every hit goes to exactly one counter of its primer, counters[p * SMX_FLANK_N_COUNTERS + ...] (uint64), tested in this order:
 *   SMX_FLANK_PRUNED       h.bbest == -2 (the barcode search was not run: orientation pruned, or a length-filtered read)
 *   SMX_FLANK_SHORT_READ   lens[i] < S
 *   SMX_FLANK_SHORT_FLANK  flen < Lb - k: no barcode can be within k of it
 *   SMX_FLANK_AMBIGUOUS    a flank byte other than upper-case A, C, G, T
 *   SMX_FLANK_COUNTED      everything else: the hit's key is counted in the table
 *   SMX_FLANK_HITS         (slot 0) the sum of the five
 *
 * Key of a counted hit (bit 0 = least significant; ~0 = empty slot, which no key equals because flen <= 26):
 *   [0, 52)   the flank, 2 bits per base, A C G T = 0 1 2 3, base t at bits [2 t, 2 t + 2), unused bits 0
 *   [52, 57)  flen
 *   57        matched: h.bbest >= 0, a panel barcode was found at this end
 *   [58, 64)  primer index p (a panel has at most 64 primers: the specimen masks are 64-bit)
 * Ends A and B of a primer share keys: the end string is orientation-normalised, so a read and its reverse complement give
 * the same keys.
 *
 *   smx_flank_create            capacity = number of slots, rounded up to a power of two (>= 8)
 *   smx_flank_accumulate_device asynchronous, ordered on `stream` behind the batch: d_windows / d_lens are what
 *                               smx_batch_run_device was given, d_hits what it dumped (all DEVICE pointers)
 *   smx_flank_read              waits for the device, then copies the occupied slots out (any order) and the counters
 *                               (n_primers * SMX_FLANK_N_COUNTERS uint64, may be NULL).  *n = number of distinct keys;
 *                               SMX_ERR_ARG when cap < *n.  If any increment found the table full, the call fails with
 *                               SMX_ERR_OVERFLOW, *dropped = the lost increments, and nothing is copied.
 *   smx_flank_clear             empty table and counters (asynchronous on `stream`)
 *
 * smx_flank_assign: stand-alone (host buffers in and out, no panel handle).  A candidate is a string of 1..26 IUPAC letters
 * as it would stand in the end string (barcode_rc) with the primer it belongs to: cands / cand_off (n_cands + 1 offsets) /
 * cand_primer.  d(c, key) = min over 0 <= j <= flen of NW(c, flank[:j]) -- edlib's SHW distance, IUPAC equalities as in
 * the demux kernels.  Per key, over the candidates of the key's primer only: best[i] = the least d that is <= k, else -1;
 * first[i] = index (caller's order) of the first candidate that attains it, else -1; ntied[i] = how many attain it.  Keys
 * may come in any order; grouped by primer (sorted, say) a wavefront walks one candidate list.  kernel_ms (may be NULL)
 * receives the device time of the kernel (HIP events).
 */
enum { SMX_FLANK_HITS = 0, SMX_FLANK_PRUNED = 1, SMX_FLANK_SHORT_READ = 2, SMX_FLANK_SHORT_FLANK = 3,
       SMX_FLANK_AMBIGUOUS = 4, SMX_FLANK_COUNTED = 5, SMX_FLANK_N_COUNTERS = 6 };
#define SMX_FLANK_MAX_W 26
#define SMX_FLANK_LEN_SHIFT 52
#define SMX_FLANK_MATCHED_SHIFT 57
#define SMX_FLANK_PRIMER_SHIFT 58

typedef struct smx_flank smx_flank;
int smx_flank_create(const smx_panel *panel, uint32_t capacity, smx_flank **out);
void smx_flank_destroy(smx_flank *flank);
int smx_flank_clear(smx_flank *flank, void *stream);
int smx_flank_accumulate_device(smx_flank *flank, void *stream, const uint8_t *d_windows, const int32_t *d_lens,
                                const smx_hit *d_hits, uint32_t n_reads);
int smx_flank_read(smx_flank *flank, uint64_t *keys, uint64_t *counts, uint32_t cap, uint32_t *n, uint64_t *counters,
                   uint64_t *dropped);
int smx_flank_assign(const uint64_t *keys, uint32_t n_keys, const char *cands, const uint32_t *cand_off,
                     const uint8_t *cand_primer, uint32_t n_cands, int32_t k, int32_t *best, int32_t *first, int32_t *ntied,
                     float *kernel_ms);

/* ---- run setup helper (host only)
 * Minimum global edit distance (exact character equality) over all pairs of the n strings seqs[off[i]..off[i+1]):
 * what setup_match_parameters derives the default barcode threshold from (reference orchestration.py:548-575,
 * edlib.align(a, b, task="distance") over itertools.combinations).  *out_min = -1 for n < 2. */
int smx_min_pairwise_distance(const char *seqs, const uint32_t *off, uint32_t n, int32_t *out_min);

#ifdef __cplusplus
}
#endif
#endif /* SMX_H */
