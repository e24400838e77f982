// smx_api.cpp -- host side of libsmx.so: panel compilation, launch glue, the C ABI of include/smx.h.
// Compiled with hipcc together with smx_kernels.hip.  No CPU implementation of the hot path lives here:
// every compute entry point needs a HIP device and fails with SMX_ERR_DEVICE otherwise.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "smx.h"
#include "smx_internal.h"
#include "smx_prescan_core.h"
#include "smx_barcode_core.h"
#include "smx_stats_core.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return fail(SMX_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// ---- IUPAC equality (reference constants.py:13-20): symmetric, NOT transitive
struct EqTable {
    bool eq[128][128];
    EqTable() {
        memset(eq, 0, sizeof(eq));
        for (int c = 0; c < 128; c++) eq[c][c] = true;
        const char *pairs[] = {"YC", "YT", "RA", "RG", "NA", "NC", "NG", "NT", "WA", "WT", "MA", "MC", "SC", "SG",
                               "KG", "KT", "BC", "BG", "BT", "DA", "DG", "DT", "HA", "HC", "HT", "VA", "VC", "VG"};
        for (const char *p : pairs) {
            eq[(int)p[0]][(int)p[1]] = true;
            eq[(int)p[1]][(int)p[0]] = true;
        }
    }
};
const EqTable &eqt() {
    static EqTable t;
    return t;
}

int code_of(unsigned char ch) {
    for (int c = 0; c < 15; c++)
        if (smx::kCodeChars[c] == (char)ch) return c;
    return 15;
}

unsigned char complement_of(unsigned char ch) {   // Bio.Seq complement, ambiguous DNA table, case kept, U->A
    static const char *from = "ACGTMRWSYKVHDBXNUacgtmrwsykvhdbxnu";
    static const char *to = "TGCAKYWSRMBDHVXNAtgcakywsrmbdhvxna";
    for (int i = 0; from[i]; i++)
        if ((unsigned char)from[i] == ch) return (unsigned char)to[i];
    return ch;
}

// bit i of peq[c] = eq(pattern[i], char of code c); code 15 never matches
bool build_peq(const char *pat, int m, unsigned long long *peq16, std::string *bad) {
    for (int c = 0; c < 16; c++) peq16[c] = 0;
    for (int i = 0; i < m; i++) {
        unsigned char pc = (unsigned char)pat[i];
        if (pc >= 128 || code_of(pc) == 15) {
            if (bad) *bad = std::string("pattern character '") + (char)pc + "' is outside the IUPAC DNA alphabet";
            return false;
        }
        for (int c = 0; c < 15; c++)
            if (eqt().eq[pc][(int)smx::kCodeChars[c]]) peq16[c] |= 1ull << i;
    }
    return true;
}

template <typename T>
size_t blob_add(std::vector<unsigned char> &blob, const std::vector<T> &v) {
    size_t off = (blob.size() + 15) & ~(size_t)15;
    blob.resize(off + std::max<size_t>(v.size() * sizeof(T), 16));
    if (!v.empty()) memcpy(blob.data() + off, v.data(), v.size() * sizeof(T));
    return off;
}

}  // namespace

#define SMX_MAX_STREAMS 16   // distinct streams one panel may be launched on

extern "C" size_t smx_packed_stride_for(int32_t S);   // smx_io.cpp
extern "C" int smx_launch_unpack_windows(void *stream, const uint8_t *d_packed, uint8_t *d_windows, uint32_t n_reads, int S,
                                         int pstride, int wstride, int n_cu);   // smx_pack.hip

struct DevBuf {   // grow-only device buffer of the host-buffer convenience path
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = n + n / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// The environment switches of a panel: none is needed in production.  This struct is the source of truth (DESIGN.md,
// section 8, has the table); read_switches fills it at every smx_panel_create, and nothing else in this file looks at the
// environment on a panel's behalf.
struct Switches {
    bool no_prescan = false;         // SMX_NO_PRESCAN: every primer alignment by the demux kernel's scalar scan
    bool no_bitslice = false;        // SMX_NO_BITSLICE: per-barcode scan instead of the bit-sliced one
    bool no_table_sharing = false;   // SMX_NO_TABLE_SHARING: one barcode table per primer even when lists repeat
    int cap_hits = 0, cap_ents = 0;  // SMX_TEST_CAPS=h,e: small barcode rounds
    int no_sp = 0;                   // SMX_NO_SPECIALISE (bit 0), SMX_NO_SPECIALISE_NP (bit 1): generic instantiations
    bool no_lean_tails = false;      // SMX_NO_LEAN_TAILS: --trim tails on the slots kernel
    bool force_slots = false;        // SMX_FORCE_SLOTS: every launch on the slots kernel
    bool debug = false;              // SMX_DEBUG: tile plan, occupancy (and placement, with phase timing) on stderr
    bool debug_overflow = false;     // SMX_DEBUG_OVERFLOW: overflow tiles of every compact launch on stderr (synchronises)
    bool phase_timing = false;       // SMX_PHASE_TIMING: per-phase cycle sums, printed when the panel is destroyed
    bool lds_budget_set = false;     // SMX_LDS_BUDGET: LDS bytes a dense tile may take (default: a quarter / a third of a CU's)
    size_t lds_budget = 0;
    int tile_r = 64;                 // SMX_TILE_R: largest dense tile tried, 1..64 reads
    size_t lds_pad = 0;              // SMX_LDS_PAD: bytes added to the lean tile's LDS request
    bool compact_off = false;        // SMX_COMPACT=0: no compact tiles
    int compact_items = -1;          // SMX_COMPACT_ITEMS: records per compact tile, 2 NP..256 (-1: unset, 256); forces compact mode
    int compact_r = 0;               // SMX_COMPACT_R: reads per compact tile, 1..64 (0: unset); forces compact mode
    int blocks_per_cu = 0;           // SMX_BLOCKS_PER_CU: grid multiplier of every demux launch, >= 1 (0: unset, occupancy)
};

static Switches read_switches() {
    Switches w;
    auto on = [](const char *name) { return getenv(name) != nullptr; };
    w.no_prescan = on("SMX_NO_PRESCAN"); w.no_bitslice = on("SMX_NO_BITSLICE"); w.no_table_sharing = on("SMX_NO_TABLE_SHARING");
    if (const char *e = getenv("SMX_TEST_CAPS")) sscanf(e, "%d,%d", &w.cap_hits, &w.cap_ents);
    w.no_sp = (on("SMX_NO_SPECIALISE") ? 1 : 0) | (on("SMX_NO_SPECIALISE_NP") ? 2 : 0);
    w.no_lean_tails = on("SMX_NO_LEAN_TAILS"); w.force_slots = on("SMX_FORCE_SLOTS");
    w.debug = on("SMX_DEBUG"); w.debug_overflow = on("SMX_DEBUG_OVERFLOW"); w.phase_timing = on("SMX_PHASE_TIMING");
    if (const char *e = getenv("SMX_LDS_BUDGET")) { w.lds_budget_set = true; w.lds_budget = (size_t)atol(e); }
    if (const char *e = getenv("SMX_TILE_R")) w.tile_r = std::max(1, std::min(64, atoi(e)));
    if (const char *e = getenv("SMX_LDS_PAD")) w.lds_pad = (size_t)atol(e);
    if (const char *e = getenv("SMX_COMPACT")) w.compact_off = atoi(e) == 0;
    if (const char *e = getenv("SMX_COMPACT_ITEMS")) w.compact_items = std::max(0, std::min(256, atoi(e)));
    if (const char *e = getenv("SMX_COMPACT_R")) w.compact_r = std::max(1, std::min(64, atoi(e)));
    if (const char *e = getenv("SMX_BLOCKS_PER_CU")) w.blocks_per_cu = std::max(1, atoi(e));
    return w;
}

using smx::TilePlan;   // one per launch mode; ensure_device fills blocks_per_cu
// lean: no per-barcode slots.  slots: --trim tails where the lean kernel cannot report the extent, parity dumps.  compact:
// tiles of the lean kernel (panels with many primers) that keep per-alignment records only for the nitems alignments the match
// words flag; a tile that needs more goes on the overflow list and is redone by a dense lean launch right behind the compact one.
enum { LEAN, SLOTS, COMPACT, N_MODES };

struct smx_panel {
    smx::DevPanel hp;                 // scalar fields valid; pointers filled at upload
    std::vector<unsigned char> blob;  // host image of the device allocation
    size_t o_ppeq, o_prpeq, o_bpeq, o_lut, o_pm, o_pk, o_pdir, o_pfidx, o_pbc_off, o_pbc, o_bm, o_pair_f, o_pair_r,
        o_pair_pool, o_bsre, o_bstab = 0, o_pairrec = 0, o_specrec = 0;
    int use64 = 0;
    Switches sw;
    TilePlan plan[N_MODES];           // plan_tiles
    int nitems = 0;                   // records per compact tile; 0: compact mode off
    // device state (lazy, one device per process)
    void *d_blob = nullptr;
    int device = -1;
    int n_cu = 0;
    std::mutex ws_mutex;                     // smx_batch_run is serialised per panel (one workspace)
    DevBuf ws[8];                            // windows, lens, ops, extra, n_extra, counts, hits, bdist
    // Launch counters {tile queue head, -, finished workgroups, extra records}, 64 bytes per slot, self re-arming.
    // One slot per stream the panel has been launched on: launches on one stream are ordered, launches on different
    // streams (double-buffered pipelines) each pull tiles from their own queue.
    unsigned *d_tile_counter = nullptr;
    std::mutex tc_mutex;
    std::vector<void *> tc_streams;          // slot -> stream (valid where tc_used)
    std::vector<char> tc_used;               // a lane gives its slot back when it is destroyed: the next new stream reuses it
    // primer prescan (smx_prescan.hip): bit-sliced HW alignment of every primer over both end windows, run in front of
    // the demux kernel, which then only redoes the alignments the prescan cannot take (smx_prescan_core.h)
    bool pre_ok = false;
    smx::PreDesc pre;
    int pre_mr = 24, pre_nx = 0, pre_blocks_t = 1, pre_blocks_d = 8;   // longest primer, degenerate symbols, residency
    size_t pre_lds = 0;                      // transpose kernel staging
    DevBuf pre_planes[SMX_MAX_STREAMS];      // per stream slot: the 2-bit text planes of the batch (read-tile major)
    DevBuf pre_recs[SMX_MAX_STREAMS];        // per stream slot: [2 * NP][search_len / 16][n_reads rounded up to a tile] flag words
    DevBuf pre_match[SMX_MAX_STREAMS];       // per stream slot: match words [tile][2 * NP][32 groups] (bit = read reaches the threshold)
    DevBuf pre_codes[SMX_MAX_STREAMS];       // per stream slot: row-major 2-bit codes [read][end][chunk] + one flag byte per read behind them
    int share = 1;      // smx_panel_set_streams: batches the caller keeps in flight on as many streams
    DevBuf ovf[SMX_MAX_STREAMS];             // per stream slot: overflow list, one entry per compact tile
    hipEvent_t kev[4] = {nullptr, nullptr, nullptr, nullptr};   // smx_debug_kernel_times: start, after transpose, after DP, end
    bool kev_on = false, kev_pre = false;
    unsigned long long *d_phase = nullptr;   // SMX_PHASE_TIMING diagnostic
    int phase_grid = 0;
};

// The tile plan of a panel (h: every scalar field set): plan[].R / .lds per mode, *nitems > 0 where compact mode is on.
static void plan_tiles(const smx::DevPanel &h, int use64, bool pre_ok, const Switches &sw, TilePlan plan[N_MODES], int *nitems) {
    // Tile size: the largest R (<= 64 reads, one scorer lane per read) whose tile fits a quarter of the CU's LDS, so that
    // four workgroups stay resident; but a tile twice as large at three workgroups per CU keeps more reads in flight
    // (6R vs 4R) and wins for panels with many primers (measured on the 8-primer panel: R = 32 x 3 beats R = 16 x 4 by 7 %,
    // R = 64 x 2 loses 45 %).  SMX_TILE_R / SMX_LDS_BUDGET override for tuning experiments.
    auto lds_blocks = [](size_t need) { return (int)(SMX_LDS_POOL / ((need + 511) & ~(size_t)511)); };   // workgroups of `need` bytes a CU holds
    const size_t budget = sw.lds_budget_set ? sw.lds_budget : (SMX_LDS_POOL / 4) & ~(size_t)511;
    for (int slots = 0; slots < 2; slots++) {
        auto pick = [&](size_t bud) {
            TilePlan t;
            for (t.R = sw.tile_r; ; t.R >>= 1) {
                t.lds = smx_demux_lds_bytes(&h, use64, t.R, slots, 0);
                if (t.lds <= bud || t.R == 1) return t;
            }
        };
        plan[slots ? SLOTS : LEAN] = pick(budget);
        if (!sw.lds_budget_set && !slots) {   // (the slots kernel measured 2.5 % slower at three workgroups per CU)
            const TilePlan t3 = pick((SMX_LDS_POOL / 3) & ~(size_t)511);
            if (t3.R > plan[LEAN].R) plan[LEAN] = t3;
        }
    }
    TilePlan &lean = plan[LEAN];
    lean.lds += sw.lds_pad;   // tuning experiment: residency vs LDS size
    // compact mode: worth it when the dense tile had to shrink (R * 2 NP records do not fit) and the prescan is there to say
    // which alignments matter.  Largest tile (multiples of 8 reads) at four workgroups per CU, or a larger one at three if
    // that keeps more reads in flight (8-primer panel: the kernel's time falls as a + b / reads in flight from R = 24 x 4 to
    // R = 64 x 3).  SMX_COMPACT=0 turns it off, SMX_COMPACT_ITEMS / SMX_COMPACT_R are test / tuning hooks.
    const bool items_set = sw.compact_items >= 0;
    const int items = items_set ? std::max(2 * h.NP, sw.compact_items) : 256;
    *nitems = 0;
    if (!pre_ok || sw.compact_off || !(lean.R < 64 || items_set)) return;
    auto need_c = [&](int R) { return smx_demux_lds_bytes(&h, use64, R, 0, items); };
    int best_R = 0, best_blocks = 0;
    size_t best_need = 0;
    for (int R = 64; R >= 8; R -= 8) {
        const size_t need = need_c(R);
        if (need > SMX_LDS_POOL) continue;
        const int blocks = std::min(4, lds_blocks(need));
        if (blocks < 3) continue;   // two workgroups per CU lose more to exposed latency than their larger tiles win back
                                    // (measured: 8-primer panel, -l 160: R = 64 x 2 is 40 % slower than R = 40 x 3)
        if (R * blocks > best_R * best_blocks) { best_R = R; best_blocks = blocks; best_need = need; }
    }
    // a tile size that has a default-flags instantiation wins over a larger generic one (wide-window stress shape:
    // 32-read tiles on `SP = 3` 1.11 ms per 10^6 reads, 48-read tiles on the generic compact kernel 1.15)
    for (int R = 64; R >= 8; R -= 8) {
        const size_t need = need_c(R);
        if (need > SMX_LDS_POOL || lds_blocks(need) < 3) continue;
        if (smx_demux_sp_query(&h, use64, 0, 1, R, items, 1) != 0) {
            if (R != best_R) { best_R = R; best_blocks = std::min(4, lds_blocks(need)); best_need = need; }
            break;
        }
    }
    if (sw.compact_r) { best_R = sw.compact_r; best_need = need_c(best_R); best_blocks = 1; }
    const int dense_blocks = std::min(4, lds_blocks(lean.lds));
    if (best_R > 0 && (best_R * best_blocks >= lean.R * dense_blocks || items_set || sw.compact_r)) {
        plan[COMPACT].R = best_R; plan[COMPACT].lds = best_need; *nitems = items;
    }
}

extern "C" {

// shared with smx_io.cpp: set the thread-local message and return `code`
int smx_set_error(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int smx_abi_version(void) { return SMX_ABI_VERSION; }
const char *smx_last_error(void) { return g_err.c_str(); }

int smx_device_init(int device, int *n_devices) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return fail(SMX_ERR_DEVICE, "no HIP device available (%s)", hipGetErrorString(e));
    if (n_devices) *n_devices = n;
    if (device < 0 || device >= n) return fail(SMX_ERR_ARG, "device %d out of range (0..%d)", device, n - 1);
    HIP_TRY(hipSetDevice(device));
    return SMX_OK;
}

int smx_panel_create(const smx_panel_desc *d, smx_panel **out) {
    if (!d || !out) return fail(SMX_ERR_ARG, "null argument");
    if (d->abi_version != SMX_ABI_VERSION) return fail(SMX_ERR_ARG, "ABI version mismatch: %u", d->abi_version);
    const int NP = (int)d->n_primers, NB = (int)d->n_barcodes, NS = (int)d->n_specimens, NPAIR = (int)d->n_pairs;
    if (NP <= 0 || NB <= 0 || NS <= 0 || NPAIR <= 0) return fail(SMX_ERR_ARG, "empty panel");
    if (NP > 64) return fail(SMX_ERR_UNSUPPORTED, "more than 64 distinct primers (%d)", NP);
    if (NPAIR > 127) return fail(SMX_ERR_UNSUPPORTED, "more than 127 primer pairs (%d)", NPAIR);
    if (NB > 4096) return fail(SMX_ERR_UNSUPPORTED, "more than 4096 distinct barcodes (%d)", NB);   // (b1, b2) table: 32 B per pair
    if (d->search_len < 1 || d->search_len > 256)
        return fail(SMX_ERR_UNSUPPORTED, "search_len %d outside 1..256", d->search_len);
    if (d->k_index < 0 || d->k_index > 32) return fail(SMX_ERR_UNSUPPORTED, "index edit distance %d outside 0..32", d->k_index);
    if (d->trim < 0 || d->trim > 3 || d->dereplicate < 0 || d->dereplicate > 1) return fail(SMX_ERR_ARG, "bad trim/dereplicate");

    smx_panel *P = new smx_panel();
    const Switches &sw = P->sw = read_switches();
    smx::DevPanel &h = P->hp;
    memset(&h, 0, sizeof(h));
    h.NP = NP; h.NB = NB; h.NS = NS; h.NPAIR = NPAIR;
    h.S = d->search_len;
    h.wstride = ((2 * h.S) + 15) & ~15;
    h.kidx = d->k_index;
    h.bmax = d->barcode_len_max;
    h.pfmin = d->prefilter_min_len;
    h.preorient = d->preorient ? 1 : 0;
    h.trim = d->trim;
    h.derep = d->dereplicate;
    h.minlen = d->min_length;
    h.maxlen = d->max_length;
    h.need_starts = (d->trim == SMX_TRIM_PRIMERS || d->trim == SMX_TRIM_TAILS || d->want_starts) ? 1 : 0;

    std::string bad;
    std::vector<unsigned long long> ppeq(NP * 16), prpeq(NP * 16);
    std::vector<int> pm(NP), pk(NP), pdir(NP), pfidx(NP), pbc_off(NP + 1);
    int maxm = 0, maxB = 1;
    for (int p = 0; p < NP; p++) {
        int a = (int)d->primer_rc_off[p], m = (int)d->primer_rc_off[p + 1] - a;
        if (m < 1 || m > 64) { delete P; return fail(SMX_ERR_UNSUPPORTED, "primer %d has length %d (supported 1..64)", p, m); }
        std::string pat(d->primer_rc + a, m), rpat(pat.rbegin(), pat.rend());
        if (!build_peq(pat.data(), m, &ppeq[p * 16], &bad) || !build_peq(rpat.data(), m, &prpeq[p * 16], &bad)) {
            delete P;
            return fail(SMX_ERR_UNSUPPORTED, "primer %d: %s", p, bad.c_str());
        }
        pm[p] = m;
        pk[p] = d->primer_k[p];
        if (pk[p] < 0 || pk[p] >= m) { delete P; return fail(SMX_ERR_UNSUPPORTED, "primer %d: edit distance %d must be in 0..len-1", p, pk[p]); }
        pdir[p] = d->primer_dir[p] ? 1 : 0;
        pfidx[p] = d->primer_file_index[p];
        if (pfidx[p] < 0 || pfidx[p] > 2000) { delete P; return fail(SMX_ERR_UNSUPPORTED, "primer file index %d outside 0..2000", pfidx[p]); }
        pbc_off[p] = (int)d->primer_bc_off[p];
        maxm = std::max(maxm, m);
        maxB = std::max(maxB, (int)(d->primer_bc_off[p + 1] - d->primer_bc_off[p]));
    }
    pbc_off[NP] = (int)d->primer_bc_off[NP];
    {   // prescan description: the searched patterns as A/C/G/T sets per row
        std::vector<std::string> pats(NP);
        std::vector<const char *> pp(NP);
        std::vector<int> pl(NP);
        for (int p = 0; p < NP; p++) {
            pats[p].assign(d->primer_rc + d->primer_rc_off[p], d->primer_rc_off[p + 1] - d->primer_rc_off[p]);
            pp[p] = pats[p].c_str();
            pl[p] = (int)pats[p].size();
        }
        memset(&P->pre, 0, sizeof(P->pre));
        P->pre_ok = maxm <= smx::PRE_MAXROWS && !sw.no_prescan &&
                    smx::prescan_build_desc(&P->pre, NP, h.S, pp.data(), pl.data(), pk.data(),
                                            [](unsigned char a, unsigned char b) { return a < 128 && b < 128 && eqt().eq[a][b]; });
        if (P->pre_ok) {
            P->pre_mr = maxm;
            P->pre_nx = P->pre.nsym - 4;
            P->pre_lds = smx_prescan_lds_bytes(h.S);
            if (P->pre_lds > 160 * 1024) P->pre_ok = false;
        }
    }
    if (maxB > 1024) { delete P; return fail(SMX_ERR_UNSUPPORTED, "more than 1024 barcodes on one primer (%d)", maxB); }
    std::vector<int> pbc(std::max(pbc_off[NP], 1));
    for (int i = 0; i < pbc_off[NP]; i++) {
        pbc[i] = (int)d->primer_bc[i];
        if (pbc[i] < 0 || pbc[i] >= NB) { delete P; return fail(SMX_ERR_ARG, "primer_bc[%d] out of range", i); }
    }
    std::vector<unsigned> bpeq(NB * 16);
    std::vector<int> bm(NB);
    for (int b = 0; b < NB; b++) {
        int a = (int)d->barcode_rc_off[b], m = (int)d->barcode_rc_off[b + 1] - a;
        if (m < 1 || m > 32) { delete P; return fail(SMX_ERR_UNSUPPORTED, "barcode %d has length %d (supported 1..32)", b, m); }
        if (d->k_index >= m) { delete P; return fail(SMX_ERR_UNSUPPORTED, "index edit distance %d >= barcode length %d", d->k_index, m); }
        unsigned long long t[16];
        if (!build_peq(d->barcode_rc + a, m, t, &bad)) { delete P; return fail(SMX_ERR_UNSUPPORTED, "barcode %d: %s", b, bad.c_str()); }
        for (int c = 0; c < 16; c++) bpeq[b * 16 + c] = (unsigned)t[c];
        bm[b] = m;
    }
    // bit-sliced barcode tables: usable when every barcode has the same length <= 16 and k <= 7
    const int MBWh = (maxB + 31) / 32;
    bool bs_ok = d->k_index <= 7 && !sw.no_bitslice;
    for (int b = 0; b < NB; b++) if (bm[b] != bm[0] || bm[b] > 16) bs_ok = false;
    std::vector<unsigned> bsre((size_t)NP * 16 * 16 * MBWh, 0u);
    if (bs_ok)
        for (int p = 0; p < NP; p++)
            for (int li = pbc_off[p]; li < pbc_off[p + 1]; li++) {
                int gb = pbc[li], bi = li - pbc_off[p];   // [primer][word][row][code]; rows past the barcode are wildcards
                smx::bs_table_add(&bsre[((size_t)p * MBWh + (bi >> 5)) * 256], bi & 31, &bpeq[gb * 16], bm[gb]);
            }
    // primers with the same barcode list (the same kit in every pool) share one table: the 8-primer panel keeps 2 of 8 in LDS
    std::vector<int> bs_tab(NP, 0);
    {
        const size_t tw = (size_t)16 * 16 * MBWh;
        std::vector<unsigned> packed;
        int nt = 0;
        for (int p = 0; p < NP; p++) {
            int found = -1;
            for (int q = 0; q < nt && found < 0; q++)
                if (std::equal(bsre.begin() + (size_t)p * tw, bsre.begin() + (size_t)(p + 1) * tw, packed.begin() + (size_t)q * tw)) found = q;
            if (found < 0) { packed.insert(packed.end(), bsre.begin() + (size_t)p * tw, bsre.begin() + (size_t)(p + 1) * tw); found = nt++; }
            bs_tab[p] = found;
        }
        if (sw.no_table_sharing) { nt = NP; for (int p = 0; p < NP; p++) bs_tab[p] = p; }   // A/B and test hook
        else bsre.swap(packed);
        h.n_bstab = nt;
    }
    h.bs_ok = bs_ok ? 1 : 0;
    h.cap_hits = sw.cap_hits; h.cap_ents = sw.cap_ents; h.no_sp = sw.no_sp;   // the switches the kernel and its glue look at
    h.bs_m = bm[0];
    if (h.pfmin != 0 && h.pfmin < 2) { delete P; return fail(SMX_ERR_UNSUPPORTED, "prefilter min length %d < 2: disable the prefilter", h.pfmin); }
    if (h.bmax + h.kidx > 200) { delete P; return fail(SMX_ERR_UNSUPPORTED, "barcode length + k too large"); }
    h.maxB = maxB;
    h.n_pbc = pbc_off[NP];
    std::vector<unsigned char> lut(512);
    for (int c = 0; c < 256; c++) {
        lut[c] = (unsigned char)code_of((unsigned char)c);
        lut[256 + c] = (unsigned char)code_of(complement_of((unsigned char)c));
    }
    std::vector<int> pair_f(NPAIR), pair_r(NPAIR), pair_pool(NPAIR);
    for (int i = 0; i < NPAIR; i++) {
        pair_f[i] = (int)d->pair_fwd[i];
        pair_r[i] = (int)d->pair_rev[i];
        pair_pool[i] = d->pair_pool[i];
        if (pair_f[i] >= NP || pair_r[i] >= NP || pdir[pair_f[i]] != 0 || pdir[pair_r[i]] != 1) {
            delete P;
            return fail(SMX_ERR_ARG, "pair %d is not (forward primer, reverse primer)", i);
        }
    }
    // (b1,b2) -> chain of specimens in file order (Specimens.specimen_for_exact_match walks file order)
    std::vector<int> pairhead((size_t)NB * NB, -1), spec_next(NS, -1), spec_pool(NS), tail((size_t)NB * NB, -1);
    std::vector<unsigned long long> p1m(NS), p2m(NS);
    for (int s = 0; s < NS; s++) {
        unsigned b1 = d->spec_b1[s], b2 = d->spec_b2[s];
        if (b1 >= (unsigned)NB || b2 >= (unsigned)NB) { delete P; return fail(SMX_ERR_ARG, "specimen %d barcode index out of range", s); }
        size_t key = (size_t)b1 * NB + b2;
        if (pairhead[key] < 0) pairhead[key] = s; else spec_next[tail[key]] = s;
        tail[key] = s;
        p1m[s] = d->spec_p1mask[s];
        p2m[s] = d->spec_p2mask[s];
        spec_pool[s] = d->spec_pool[s];
    }
    auto &B = P->blob;
    P->o_ppeq = blob_add(B, ppeq); P->o_prpeq = blob_add(B, prpeq); P->o_bpeq = blob_add(B, bpeq); P->o_lut = blob_add(B, lut);
    P->o_pm = blob_add(B, pm); P->o_pk = blob_add(B, pk); P->o_pdir = blob_add(B, pdir); P->o_pfidx = blob_add(B, pfidx);
    P->o_pbc_off = blob_add(B, pbc_off); P->o_pbc = blob_add(B, pbc); P->o_bm = blob_add(B, bm);
    P->o_pair_f = blob_add(B, pair_f); P->o_pair_r = blob_add(B, pair_r); P->o_pair_pool = blob_add(B, pair_pool);
    {   // packed lookup tables (32 bytes per barcode pair)
        std::vector<smx::SpecRec> specrec(NS), pairrec((size_t)NB * NB);
        for (int s2 = 0; s2 < NS; s2++) specrec[s2] = {p1m[s2], p2m[s2], s2, spec_next[s2], spec_pool[s2], 0};
        for (size_t k2 = 0; k2 < pairrec.size(); k2++)
            pairrec[k2] = pairhead[k2] >= 0 ? specrec[pairhead[k2]] : smx::SpecRec{0ull, 0ull, -1, -1, -1, 0};
        P->o_pairrec = blob_add(B, pairrec); P->o_specrec = blob_add(B, specrec);
    }
    P->o_bsre = blob_add(B, bsre);
    P->o_bstab = blob_add(B, bs_tab);

    P->use64 = maxm > 32 ? 1 : 0;
    plan_tiles(h, P->use64, P->pre_ok, sw, P->plan, &P->nitems);
    if (P->plan[LEAN].lds > 160 * 1024 || P->plan[SLOTS].lds > 160 * 1024) {
        const size_t need = std::max(P->plan[LEAN].lds, P->plan[SLOTS].lds);
        delete P;
        return fail(SMX_ERR_UNSUPPORTED, "panel needs %zu bytes of LDS per read tile", need);
    }
    *out = P;
    return SMX_OK;
}

void smx_panel_destroy(smx_panel *P) {
    if (!P) return;
    if (P->d_phase) {   // diagnostic: print the per-phase share of block cycles
        std::vector<unsigned long long> h((size_t)P->phase_grid * 16);
        if (hipMemcpy(h.data(), P->d_phase, h.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            unsigned long long sum[10] = {0}, tot = 0;
            for (int b = 0; b < P->phase_grid; b++)
                for (int i = 0; i < 10; i++) { sum[i] += h[(size_t)b * 16 + i]; tot += h[(size_t)b * 16 + i]; }
            const char *names[8] = {"zero+barrier", "primer_scan", "orient+scan", "entries", "barcode_scan", "summary",
                                    "scorer||encode", "store"};
            fprintf(stderr, "[smx phase timing] R=%d lds=%zu blocks/CU=%d:", P->plan[LEAN].R, P->plan[LEAN].lds, P->plan[LEAN].blocks_per_cu);
            tot -= sum[8] + sum[9];   // [8] = the first encode wave's own encode time (inside the scorer||encode region), [9] = the scorer wave's own time
            for (int i = 0; i < 8; i++) fprintf(stderr, " %s=%.1f%%", names[i], tot ? 100.0 * sum[i] / tot : 0.0);
            fprintf(stderr, " (inside the region: scorer wave %.1f%%, first encode wave %.1f%%)", tot ? 100.0 * sum[9] / tot : 0.0, tot ? 100.0 * sum[8] / tot : 0.0);
            fprintf(stderr, "\n");
            if (P->sw.debug) {   // where did wave w of each workgroup land?  hist[w][simd]
                unsigned long long worked = 0;
                for (int b = 0; b < P->phase_grid; b++) worked += h[(size_t)b * 16 + 14];
                fprintf(stderr, "[smx placement] workgroup-launches that processed at least one tile: %llu (grid %d)\n", worked, P->phase_grid);
                int hist[4][4] = {{0}};
                for (int b = 0; b < P->phase_grid; b++)
                    for (int w = 0; w < 4; w++) hist[w][(h[(size_t)b * 16 + 10 + w] >> 4) & 3]++;
                for (int w = 0; w < 4; w++)
                    fprintf(stderr, "[smx placement] wave %d on simd 0..3: %d %d %d %d\n", w, hist[w][0], hist[w][1], hist[w][2], hist[w][3]);
                for (int b = 0; b < 12 && b < P->phase_grid; b++) {
                    unsigned v = (unsigned)h[(size_t)b * 16 + 10];
                    fprintf(stderr, "[smx placement] block %d wave0: slot %u simd %u cu %u sh %u se %u\n", b, v & 15, (v >> 4) & 3, (v >> 8) & 15, (v >> 12) & 1, (v >> 13) & 7);
                }
            }
        }
        (void)hipFree(P->d_phase);
    }
    if (P->d_blob) (void)hipFree(P->d_blob);
    if (P->d_tile_counter) (void)hipFree(P->d_tile_counter);
    for (auto &b : P->ws) b.release();
    for (auto &b : P->pre_recs) b.release();
    for (auto &b : P->pre_match) b.release();
    for (auto &b : P->pre_codes) b.release();
    for (auto &b : P->ovf) b.release();
    for (auto &b : P->pre_planes) b.release();
    for (auto &e : P->kev) if (e) (void)hipEventDestroy(e);
    delete P;
}

size_t smx_counts_len(const smx_panel *P) { return P ? (size_t)SMX_CNT_SPECIMEN0 + P->hp.NS : 0; }
size_t smx_window_stride(const smx_panel *P) { return P ? (size_t)P->hp.wstride : 0; }
size_t smx_packed_stride(const smx_panel *P) { return P ? smx_packed_stride_for(P->hp.S) : 0; }
size_t smx_hits_per_read(const smx_panel *P) { return P ? (size_t)2 * P->hp.NP : 0; }
size_t smx_bdist_per_read(const smx_panel *P) { return P ? (size_t)2 * P->hp.NP * P->hp.maxB : 0; }

int smx_pack_windows(const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, int32_t S, uint8_t *windows,
                     int32_t *lens) {
    if (!bases || !offsets || !windows || !lens || S < 1) return fail(SMX_ERR_ARG, "null argument");
    const size_t stride = ((size_t)(2 * S) + 15) & ~(size_t)15;
    for (uint32_t i = 0; i < n_reads; i++) {
        uint64_t a = offsets[i], b = offsets[i + 1];
        if (b < a || b - a > 0x7FFFFFFFull) return fail(SMX_ERR_ARG, "read %u: bad offsets", i);
        int L = (int)(b - a), Sp = L < S ? L : S;
        uint8_t *w = windows + (size_t)i * stride;
        memset(w, 0, stride);
        memcpy(w, bases + a, (size_t)Sp);
        memcpy(w + S, bases + b - Sp, (size_t)Sp);
        lens[i] = L;
    }
    return SMX_OK;
}

// The launch-counter slot of `stream` on this panel (-1: none / no free slot).  claim: take a free slot for a new stream.
static int stream_slot(smx_panel *P, void *stream, bool claim) {
    std::lock_guard<std::mutex> g(P->tc_mutex);
    int free_slot = -1;
    for (size_t i = 0; i < P->tc_streams.size(); i++) {
        if (P->tc_used[i] && P->tc_streams[i] == stream) return (int)i;
        if (!P->tc_used[i] && free_slot < 0) free_slot = (int)i;
    }
    if (!claim) return -1;
    if (free_slot < 0) {
        if (P->tc_streams.size() == SMX_MAX_STREAMS) return -1;
        P->tc_streams.push_back(stream);
        P->tc_used.push_back(1);
        return (int)P->tc_streams.size() - 1;
    }
    P->tc_streams[free_slot] = stream;
    P->tc_used[free_slot] = 1;
    return free_slot;
}

// A stream is going away (synchronised by the caller): its slot -- counters and prescan buffers -- is free for the next one.
static void stream_release(smx_panel *P, void *stream) {
    std::lock_guard<std::mutex> g(P->tc_mutex);
    for (size_t i = 0; i < P->tc_streams.size(); i++)
        if (P->tc_used[i] && P->tc_streams[i] == stream) P->tc_used[i] = 0;
}

// After a failed or out-of-step launch on `stream` (already synchronised): re-arm THAT stream's launch counters only.
// Other lanes of the panel may have kernels in flight on their own slots.
static void stream_reset_counters(smx_panel *P, void *stream) {
    const int sl = stream_slot(P, stream, false);
    if (sl >= 0 && P->d_tile_counter) (void)hipMemset(P->d_tile_counter + 16 * sl, 0, 64);
}

static int ensure_device(smx_panel *P) {
    if (P->d_blob) return SMX_OK;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(SMX_ERR_DEVICE, "libsmx has no CPU path: no HIP device available (%s)", hipGetErrorString(e));
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    P->device = dev;
    P->n_cu = prop.multiProcessorCount;
    HIP_TRY(hipMalloc(&P->d_blob, P->blob.size()));
    HIP_TRY(hipMemcpy(P->d_blob, P->blob.data(), P->blob.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc((void **)&P->d_tile_counter, 64 * SMX_MAX_STREAMS));
    HIP_TRY(hipMemset(P->d_tile_counter, 0, 64 * SMX_MAX_STREAMS));   // the kernel re-arms these counters itself after every launch
    unsigned char *b = (unsigned char *)P->d_blob;
    smx::DevPanel &h = P->hp;
    h.ppeq = (const unsigned long long *)(b + P->o_ppeq);
    h.prpeq = (const unsigned long long *)(b + P->o_prpeq);
    h.bpeq = (const unsigned *)(b + P->o_bpeq);
    h.lut = b + P->o_lut;
    h.pm = (const int *)(b + P->o_pm); h.pk = (const int *)(b + P->o_pk);
    h.pdir = (const int *)(b + P->o_pdir); h.pfidx = (const int *)(b + P->o_pfidx);
    h.pbc_off = (const int *)(b + P->o_pbc_off); h.pbc = (const int *)(b + P->o_pbc); h.bm = (const int *)(b + P->o_bm);
    h.pair_f = (const int *)(b + P->o_pair_f); h.pair_r = (const int *)(b + P->o_pair_r);
    h.pair_pool = (const int *)(b + P->o_pair_pool);
    h.pairrec = (const smx::SpecRec *)(b + P->o_pairrec);
    h.specrec = (const smx::SpecRec *)(b + P->o_specrec);
    h.bs_re = (const unsigned *)(b + P->o_bsre);
    h.bs_tab = (const int *)(b + P->o_bstab);
    const size_t lim = std::max(std::max(P->plan[LEAN].lds, P->plan[SLOTS].lds), P->plan[COMPACT].lds);
    if (lim > 64 * 1024 && smx_set_demux_lds_limit(P->use64, lim) != 0)
        return fail(SMX_ERR_DEVICE, "cannot raise the dynamic LDS limit to %zu bytes", lim);
    // persistent grid = exactly the resident workgroups (tiles are pulled from a queue): a workgroup that starts
    // after the queue has drained would only pay the panel staging and its one-time register spills
    auto occupancy = [&](int m, int *occ) {   // (behind a compact launch the dense lean kernel runs as the redo instantiation)
        const int cm = m == COMPACT ? 1 : (m == LEAN && P->nitems > 0 ? 2 : 0);
        return smx_query_occupancy(&P->hp, P->use64, m == SLOTS, cm, P->plan[m].R, m == COMPACT ? P->nitems : 0, P->plan[m].lds, occ,
                                   P->pre_ok ? 1 : 0);
    };
    for (int m = 0; m < N_MODES; m++) {
        int occ = 0;
        if (m == COMPACT && P->nitems == 0) continue;
        if (occupancy(m, &occ) != 0 || occ < 1) occ = 4;
        P->plan[m].blocks_per_cu = occ;
    }
    if (P->pre_ok) {
        if (P->pre_lds > 64 * 1024 && smx_prescan_set_lds_limit(P->pre_lds) != 0)
            return fail(SMX_ERR_DEVICE, "cannot raise the prescan kernel's dynamic LDS limit to %zu bytes", P->pre_lds);
        int occ_t = 0, occ_d = 0;
        if (smx_prescan_occupancy(P->hp.S, P->pre_mr, P->pre_nx, P->pre_lds, &occ_t, &occ_d) != 0 || occ_t < 1 || occ_d < 1) { occ_t = 1; occ_d = 8; }
        P->pre_blocks_t = occ_t;
        P->pre_blocks_d = occ_d;
        if (P->sw.debug) fprintf(stderr, "[smx] prescan: transpose %d workgroups/CU (lds %zu), DP %d waves/CU\n", occ_t, P->pre_lds, occ_d);
    }
    if (P->sw.blocks_per_cu)
        for (TilePlan &t : P->plan) t.blocks_per_cu = P->sw.blocks_per_cu;
    const TilePlan &lean = P->plan[LEAN], &slots = P->plan[SLOTS], &comp = P->plan[COMPACT];
    if (P->sw.debug) {
        int occ = -1;
        (void)occupancy(LEAN, &occ);
        fprintf(stderr, "[smx] lean R=%d lds=%zu | slots R=%d lds=%zu | occupancy API (lean): %d blocks/CU, grid multiplier %d, CUs %d\n",
                lean.R, lean.lds, slots.R, slots.lds, occ, lean.blocks_per_cu, P->n_cu);
        if (P->nitems > 0)
            fprintf(stderr, "[smx] compact lean tiles: R=%d, %d records, lds=%zu, %d blocks/CU (overflow tiles redone dense)\n", comp.R,
                    P->nitems, comp.lds, comp.blocks_per_cu);
    }
    if (P->sw.phase_timing) {
        P->phase_grid = P->n_cu * std::max(std::max(lean.blocks_per_cu, slots.blocks_per_cu), comp.blocks_per_cu);
        HIP_TRY(hipMalloc((void **)&P->d_phase, (size_t)P->phase_grid * 16 * 8));
        HIP_TRY(hipMemset(P->d_phase, 0, (size_t)P->phase_grid * 16 * 8));
        h.dbg_phase = P->d_phase;
    }
    return SMX_OK;
}

int smx_batch_run_device(const smx_panel *Pc, void *stream, const uint8_t *d_windows, const int32_t *d_lens,
                         uint32_t n_reads, smx_op *d_ops, smx_op *d_extra, uint32_t extra_cap, uint32_t *d_n_extra,
                         uint64_t *d_counts, smx_hit *d_hits, int8_t *d_bdist) {
    smx_panel *P = const_cast<smx_panel *>(Pc);
    if (!P || !d_windows || !d_lens || !d_ops || !d_n_extra || !d_counts) return fail(SMX_ERR_ARG, "null argument");
    if (extra_cap && !d_extra) return fail(SMX_ERR_ARG, "extra_cap without extra buffer");
    if (((uintptr_t)d_windows & 15) != 0) return fail(SMX_ERR_ARG, "window buffer must be 16-byte aligned");
    int rc = ensure_device(P);
    if (rc) return rc;
    if (n_reads == 0) {   // nothing to launch: the count the kernel would have written
        if (hipMemsetAsync(d_n_extra, 0, sizeof(uint32_t), (hipStream_t)stream) != hipSuccess)
            return fail(SMX_ERR_DEVICE, "cannot clear the extra-record counter");
        return SMX_OK;
    }
    // slots mode keeps one result slot per (hit, barcode): needed for the per-barcode distance dump (d_bdist) and for
    // --trim tails when the bit-sliced scan cannot report the tail extent (it can for k <= 3 and at most 32 barcodes
    // per primer).  The hit dump alone (d_hits) comes from whichever kernel the flags select, so that the parity tests
    // see the hit table of the kernel that is benchmarked; its tail_end is defined only where that kernel computes it.
    const bool lean_tails = P->hp.bs_ok && P->hp.kidx < 4 && P->hp.maxB <= 32 && !P->sw.no_lean_tails;
    const int use_slots = ((P->hp.trim == SMX_TRIM_TAILS && !lean_tails) || d_bdist || P->sw.force_slots) ? 1 : 0;
    const bool compact = !use_slots && P->nitems > 0 && P->pre_ok;
    const TilePlan &dense = P->plan[use_slots ? SLOTS : LEAN], &comp = P->plan[COMPACT];
    const int sl = stream_slot(P, stream, true);
    if (sl < 0) return fail(SMX_ERR_UNSUPPORTED, "one panel launched on more than %d streams at a time", SMX_MAX_STREAMS);
    const size_t slot = (size_t)sl;
    unsigned *tc = P->d_tile_counter + 16 * slot;
    // primer prescan in front of the demux kernel (same stream: ordered)
    const unsigned *d_pre = nullptr, *d_codes2 = nullptr;
    const uint8_t *d_naflag = nullptr;
    uint32_t npad = 0;
    if (P->kev_on) { (void)hipEventRecord(P->kev[0], (hipStream_t)stream); P->kev_pre = P->pre_ok; }
    if (P->pre_ok) {
        npad = (n_reads + smx::PRE_TILE - 1) / smx::PRE_TILE * smx::PRE_TILE;
        const size_t need = (size_t)2 * P->hp.NP * (P->hp.S >> 4) * npad * sizeof(unsigned);
        DevBuf &pb = P->pre_recs[slot], &pp = P->pre_planes[slot], &pm = P->pre_match[slot], &ov = P->ovf[slot];
        const size_t need_planes = (size_t)(npad / smx::PRE_TILE) * (P->hp.S >> 4) * 8 * 64 * 4 * sizeof(unsigned);
        const size_t need_match = P->nitems > 0 ? (size_t)(npad / smx::PRE_TILE) * 2 * P->hp.NP * smx::PRE_G * sizeof(unsigned) : 0;
        const size_t need_ovf = compact ? ((size_t)n_reads / comp.R + 2) * sizeof(unsigned) : 0;
        DevBuf &pc = P->pre_codes[slot];
        const size_t codes_bytes = (size_t)npad * 2 * (P->hp.S >> 4) * sizeof(unsigned);   // 2-bit codes, then the flag bytes
        const size_t need_codes = codes_bytes + npad;
        if (need > pb.cap || need_planes > pp.cap || need_match > pm.cap || need_ovf > ov.cap || need_codes > pc.cap) {
            if (pb.p || pp.p) (void)hipStreamSynchronize((hipStream_t)stream);   // earlier launches on this stream still use them
            hipError_t pe = pb.ensure(need);
            if (pe == hipSuccess) pe = pp.ensure(need_planes);
            if (pe == hipSuccess) pe = pc.ensure(need_codes);
            if (pe == hipSuccess && need_match) pe = pm.ensure(need_match);
            if (pe == hipSuccess && need_ovf) pe = ov.ensure(need_ovf);
            if (pe != hipSuccess) return fail(SMX_ERR_DEVICE, "prescan buffers: %s", hipGetErrorString(pe));
        }
        const uint32_t ptiles = npad / smx::PRE_TILE;
        // one workgroup per 256-read sub-tile (a few microseconds of work each): the hardware hands them out as slots free up,
        // which balances better than ~2.3 loop iterations per resident workgroup
        const int grid_t = (int)(ptiles * (smx::PRE_G / smx::PRE_SUBG));
        // (DP work items come in groups of 8 tiles x NP primers; grid a multiple of 8: blocks b and b + 8 share an XCD)
        const int grid_d = (int)std::min<uint32_t>(((ptiles + 7) / 8) * 8 * (uint32_t)P->hp.NP, (uint32_t)(P->n_cu * P->pre_blocks_d));
        d_codes2 = (const unsigned *)pc.p;
        d_naflag = (const uint8_t *)pc.p + codes_bytes;
        int pe = smx_launch_prescan(&P->pre, P->pre_mr, P->pre_nx, grid_t, P->pre_lds, grid_d, stream, d_windows, d_lens, n_reads,
                                    P->hp.wstride, (unsigned *)pp.p, (unsigned *)pb.p, P->nitems > 0 ? (unsigned *)pm.p : nullptr,
                                    P->kev_on ? (void *)P->kev[1] : nullptr, (unsigned *)pc.p, (uint8_t *)pc.p + codes_bytes);
        if (pe != 0) return fail(SMX_ERR_DEVICE, "prescan kernel launch failed: %s", hipGetErrorString((hipError_t)pe));
        d_pre = (const unsigned *)pb.p;
        if (P->kev_on) (void)hipEventRecord(P->kev[2], (hipStream_t)stream);
    }
    // (batches in flight on several streams share the CUs' workgroup slots: each demux launch takes its part of them, so
    // that the next batch's memory-bound and VALU-bound prescan kernels run beside this batch's latency-bound demux kernel)
    auto grid_of = [&](const TilePlan &t) {
        int per = std::max(1, (t.blocks_per_cu + P->share - 1) / P->share);
        // two launches side by side must not claim more slots than the CU has: nothing of the next batch's prescan kernels
        // would fit beside them (five slots, two streams: 3 + 3 measured 0.335 ms per step, 2 + 2 0.306-0.319)
        if (P->share == 2 && per * 2 > t.blocks_per_cu) per = std::max(1, t.blocks_per_cu / 2);
        return (int)std::min<uint32_t>((n_reads + t.R - 1) / t.R, (uint32_t)(P->n_cu * per));
    };
    const smx::DemuxBatch batch = {d_windows, d_lens, n_reads, d_ops, d_extra, extra_cap, d_n_extra, d_counts, d_hits, d_bdist,
                                   stream, tc, d_pre, npad};
    auto launch = [&](const TilePlan &t, int grid, const smx::DemuxAux &ax) {
        return smx_launch_demux(&P->hp, P->use64, use_slots, &t, grid, &batch, &ax);
    };
    int e;
    if (compact) {
        // compact launch over all reads, then the dense launch over the reads of the tiles it put on the overflow list
        // (usually none: its workgroups find an empty list and leave)
        e = launch(comp, grid_of(comp), {(const unsigned *)P->pre_match[slot].p, (unsigned *)P->ovf[slot].p, P->nitems, 0, comp.R, 1, d_codes2, d_naflag});
        if (e == 0 && P->sw.debug_overflow) {   // diagnostic: how many compact tiles went on the overflow list
            unsigned n_ovf = 0;
            (void)hipMemcpyAsync(&n_ovf, tc + 1, sizeof(unsigned), hipMemcpyDeviceToHost, (hipStream_t)stream);
            (void)hipStreamSynchronize((hipStream_t)stream);
            fprintf(stderr, "[smx] compact launch: %u of %u tiles left to the redo launch\n", n_ovf, (n_reads + comp.R - 1) / comp.R);
        }
        // the redo launch usually finds an empty list: one workgroup per CU is enough to start with (its workgroups
        // loop over the list), and an empty 256-workgroup launch costs less than an empty full-residency one
        if (e == 0) e = launch(dense, std::min(grid_of(dense), P->n_cu), {nullptr, (unsigned *)P->ovf[slot].p, 0, 1, comp.R, 0, d_codes2, d_naflag});
    } else {
        e = launch(dense, grid_of(dense), {nullptr, nullptr, 0, 0, 0, 0, d_codes2, d_naflag});
    }
    if (e != 0) return fail(SMX_ERR_DEVICE, "demux kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    if (P->kev_on) (void)hipEventRecord(P->kev[3], (hipStream_t)stream);
    return SMX_OK;
}

int smx_unpack_windows_device(const smx_panel *Pc, void *stream, const uint8_t *d_packed, uint32_t n_reads, uint8_t *d_windows) {
    smx_panel *P = const_cast<smx_panel *>(Pc);
    if (!P || !d_packed || !d_windows) return fail(SMX_ERR_ARG, "null argument");
    if (((uintptr_t)d_packed & 3) != 0 || ((uintptr_t)d_windows & 15) != 0) return fail(SMX_ERR_ARG, "window buffers must be 16-byte aligned");
    int rc = ensure_device(P);
    if (rc) return rc;
    int e = smx_launch_unpack_windows(stream, d_packed, d_windows, n_reads, P->hp.S, (int)smx_packed_stride_for(P->hp.S), P->hp.wstride, P->n_cu);
    if (e != 0) return fail(SMX_ERR_DEVICE, "unpack kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    return SMX_OK;
}

int smx_panel_set_streams(smx_panel *P, int n_streams) {
    if (!P || n_streams < 1 || n_streams > SMX_MAX_STREAMS) return fail(SMX_ERR_ARG, "n_streams outside 1..%d", SMX_MAX_STREAMS);
    P->share = n_streams;
    return SMX_OK;
}

int smx_debug_kernel_times(smx_panel *P, int enable, float ms[3]) {
    if (!P) return fail(SMX_ERR_ARG, "null argument");
    if (ms) {
        ms[0] = ms[1] = ms[2] = 0.f;
        if (P->kev_on && P->kev[3]) {
            HIP_TRY(hipEventSynchronize(P->kev[3]));
            if (P->kev_pre) {
                HIP_TRY(hipEventElapsedTime(&ms[0], P->kev[0], P->kev[1]));
                HIP_TRY(hipEventElapsedTime(&ms[1], P->kev[1], P->kev[2]));
                HIP_TRY(hipEventElapsedTime(&ms[2], P->kev[2], P->kev[3]));
            } else {
                HIP_TRY(hipEventElapsedTime(&ms[2], P->kev[0], P->kev[3]));
            }
        }
    }
    if (enable && !P->kev[0]) {
        int rc = ensure_device(P);
        if (rc) return rc;
        for (auto &e : P->kev) HIP_TRY(hipEventCreate(&e));
    }
    P->kev_on = enable != 0;
    return SMX_OK;
}

int smx_batch_run(const smx_panel *Pc, const uint8_t *windows, const int32_t *lens, uint32_t n_reads, smx_op *ops,
                  smx_op *extra, uint32_t extra_cap, uint32_t *n_extra, uint64_t *counts, smx_hit *hits, int8_t *bdist) {
    smx_panel *P = const_cast<smx_panel *>(Pc);
    if (!P || !windows || !lens || !ops || !n_extra || !counts) return fail(SMX_ERR_ARG, "null argument");
    int rc = ensure_device(P);
    if (rc) return rc;
    *n_extra = 0;
    if (n_reads == 0) return SMX_OK;
    const size_t wbytes = (size_t)n_reads * P->hp.wstride, ncnt = smx_counts_len(P);
    const size_t hbytes = hits ? (size_t)n_reads * smx_hits_per_read(P) * sizeof(smx_hit) : 0;
    const size_t bbytes = bdist ? (size_t)n_reads * smx_bdist_per_read(P) : 0;
    std::lock_guard<std::mutex> guard(P->ws_mutex);
#define TRY_C(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return fail(SMX_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); } while (0)
    TRY_C(P->ws[0].ensure(wbytes));
    TRY_C(P->ws[1].ensure((size_t)n_reads * 4));
    TRY_C(P->ws[2].ensure((size_t)n_reads * sizeof(smx_op)));
    TRY_C(P->ws[3].ensure(std::max<size_t>((size_t)extra_cap * sizeof(smx_op), 32)));
    TRY_C(P->ws[4].ensure(16));
    TRY_C(P->ws[5].ensure(ncnt * 8));
    if (hits) TRY_C(P->ws[6].ensure(hbytes));
    if (bdist) TRY_C(P->ws[7].ensure(bbytes));
    unsigned char *dw = (unsigned char *)P->ws[0].p, *dl = (unsigned char *)P->ws[1].p, *dop = (unsigned char *)P->ws[2].p,
                  *dex = (unsigned char *)P->ws[3].p, *dn = (unsigned char *)P->ws[4].p, *dc = (unsigned char *)P->ws[5].p,
                  *dh = hits ? (unsigned char *)P->ws[6].p : nullptr, *db = bdist ? (unsigned char *)P->ws[7].p : nullptr;
    TRY_C(hipMemcpy(dw, windows, wbytes, hipMemcpyHostToDevice));
    TRY_C(hipMemcpy(dl, lens, (size_t)n_reads * 4, hipMemcpyHostToDevice));
    TRY_C(hipMemset(dn, 0, 16));
    TRY_C(hipMemset(dc, 0, ncnt * 8));
    rc = smx_batch_run_device(P, nullptr, dw, (const int32_t *)dl, n_reads, (smx_op *)dop, (smx_op *)dex, extra_cap,
                              (uint32_t *)dn, (uint64_t *)dc, (smx_hit *)dh, (int8_t *)db);
    if (rc) return rc;
    {
        hipError_t se = hipDeviceSynchronize();
        if (se != hipSuccess) {   // an aborted launch leaves the self re-arming counters in an unknown state
            stream_reset_counters(P, nullptr);
            return fail(SMX_ERR_DEVICE, "demux kernel failed: %s", hipGetErrorString(se));
        }
    }
    std::vector<uint64_t> c(ncnt);
    TRY_C(hipMemcpy(ops, dop, (size_t)n_reads * sizeof(smx_op), hipMemcpyDeviceToHost));
    TRY_C(hipMemcpy(n_extra, dn, 4, hipMemcpyDeviceToHost));
    TRY_C(hipMemcpy(c.data(), dc, ncnt * 8, hipMemcpyDeviceToHost));
    if (extra && extra_cap)
        TRY_C(hipMemcpy(extra, dex, (size_t)std::min<uint32_t>(*n_extra, extra_cap) * sizeof(smx_op), hipMemcpyDeviceToHost));
    if (hits) TRY_C(hipMemcpy(hits, dh, hbytes, hipMemcpyDeviceToHost));
    if (bdist) TRY_C(hipMemcpy(bdist, db, bbytes, hipMemcpyDeviceToHost));
#undef TRY_C
    if (c[SMX_CNT_TOTAL] != n_reads) {
        // every read is counted exactly once by the tile that scored it: anything else means tiles were skipped or
        // repeated (a tile queue that did not start at zero) and the records above cannot be trusted
        stream_reset_counters(P, nullptr);
        return fail(SMX_ERR_DEVICE, "demux kernel processed %llu of %u reads (tile queue out of step); counters reset",
                    (unsigned long long)c[SMX_CNT_TOTAL], n_reads);
    }
    for (size_t i = 0; i < ncnt; i++) counts[i] += c[i];
    if (c[SMX_CNT_OVERFLOW]) return fail(SMX_ERR_OVERFLOW, "%llu read(s) produced more than 65535 write operations",
                                         (unsigned long long)c[SMX_CNT_OVERFLOW]);
    if (*n_extra > extra_cap) return fail(SMX_ERR_OVERFLOW, "extra buffer too small: need %u records, have %u", *n_extra, extra_cap);
    return SMX_OK;
}

int smx_align(const char *query, int qlen, const char *target, int tlen, int k, int mode, int *dist, int *starts,
              int *ends, int cap, int *nloc) {
    if (!query || !target || !dist || !nloc) return fail(SMX_ERR_ARG, "null argument");
    if (qlen < 1 || qlen > 64) return fail(SMX_ERR_UNSUPPORTED, "query length %d outside 1..64", qlen);
    if (mode != 0 && mode != 1) return fail(SMX_ERR_UNSUPPORTED, "mode %d (0 = HW, 1 = SHW)", mode);
    if (tlen < 1) return fail(SMX_ERR_UNSUPPORTED, "empty target");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(SMX_ERR_DEVICE, "libsmx has no CPU path: no HIP device");
    unsigned long long peq[32];
    std::string bad, q(query, qlen), rq(q.rbegin(), q.rend());
    if (!build_peq(q.data(), qlen, peq, &bad) || !build_peq(rq.data(), qlen, peq + 16, &bad))
        return fail(SMX_ERR_UNSUPPORTED, "%s", bad.c_str());
    std::vector<unsigned char> codes(tlen);
    for (int i = 0; i < tlen; i++) codes[i] = (unsigned char)code_of((unsigned char)target[i]);
    unsigned char *d = nullptr;
    size_t o_codes = 256, o_flag = o_codes + ((tlen + 15) & ~15), o_starts = o_flag + ((tlen + 15) & ~15),
           o_dist = o_starts + (size_t)tlen * 4, total = o_dist + 16;
    HIP_TRY(hipMalloc((void **)&d, total));
    hipError_t e = hipMemcpy(d, peq, 256, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + o_codes, codes.data(), tlen, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = (hipError_t)smx_launch_align(nullptr, (unsigned long long *)d, (unsigned long long *)d + 16, qlen, d + o_codes,
                                         tlen, k, mode, (int *)(d + o_dist), d + o_flag, (int *)(d + o_starts));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    std::vector<unsigned char> flag(tlen);
    std::vector<int> st(tlen);
    if (e == hipSuccess) e = hipMemcpy(dist, d + o_dist, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(flag.data(), d + o_flag, tlen, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(st.data(), d + o_starts, (size_t)tlen * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(SMX_ERR_DEVICE, "smx_align: %s", hipGetErrorString(e));
    int cnt = 0;
    if (*dist >= 0)
        for (int j = 0; j < tlen; j++)
            if (flag[j]) {
                if (cnt < cap && starts && ends) { starts[cnt] = st[j]; ends[cnt] = j; }
                cnt++;
            }
    *nloc = cnt;
    return SMX_OK;
}

// ---- batched alignments: grow-only device workspace shared by all calls (serialised)
namespace {
std::mutex g_align_mutex;
DevBuf g_align_ws[12];
}

int smx_align_batch(const char *queries, const uint32_t *qoff, uint32_t n_queries, const char *targets, const uint64_t *toff,
                    const uint32_t *qidx, const int32_t *k, const uint8_t *mode, uint32_t n, int32_t *dist, int32_t *nloc,
                    int32_t *starts, int32_t *ends, uint32_t cap) {
    if (!queries || !qoff || !targets || !toff || !qidx || !k || !mode || !dist || !nloc || (cap && (!starts || !ends)))
        return fail(SMX_ERR_ARG, "null argument");
    if (n == 0) return SMX_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SMX_ERR_DEVICE, "libsmx has no CPU path: no HIP device");
    std::vector<unsigned long long> qpeq((size_t)n_queries * 32);
    std::vector<int> qlen(n_queries);
    std::string bad;
    for (uint32_t q = 0; q < n_queries; q++) {
        const int m = (int)(qoff[q + 1] - qoff[q]);
        if (m < 1 || m > 64) return fail(SMX_ERR_UNSUPPORTED, "query %u: length %d outside 1..64", q, m);
        std::string s(queries + qoff[q], m), r(s.rbegin(), s.rend());
        if (!build_peq(s.data(), m, &qpeq[(size_t)q * 32], &bad) || !build_peq(r.data(), m, &qpeq[(size_t)q * 32 + 16], &bad))
            return fail(SMX_ERR_UNSUPPORTED, "query %u: %s", q, bad.c_str());
        qlen[q] = m;
    }
    const uint64_t tbytes = toff[n];
    std::vector<unsigned char> codes(tbytes);
    for (uint32_t i = 0; i < n; i++) {
        if (toff[i + 1] <= toff[i]) return fail(SMX_ERR_UNSUPPORTED, "alignment %u: empty target", i);
        if (qidx[i] >= n_queries || mode[i] > 1) return fail(SMX_ERR_ARG, "alignment %u: bad query index or mode", i);
        if (k[i] < 0 || k[i] > 250) return fail(SMX_ERR_ARG, "alignment %u: bad max distance", i);
    }
    for (uint64_t j = 0; j < tbytes; j++) codes[j] = (unsigned char)code_of((unsigned char)targets[j]);
    std::lock_guard<std::mutex> guard(g_align_mutex);
    DevBuf *B = g_align_ws;
    const size_t sz[11] = {qpeq.size() * 8, qlen.size() * 4, (size_t)n * 4, (size_t)tbytes, ((size_t)n + 1) * 8, (size_t)n * 4, (size_t)n,
                           (size_t)tbytes, (size_t)n * 4, (size_t)n * 4, (size_t)n * cap * 4};
    for (int b = 0; b < 11; b++) HIP_TRY(B[b].ensure(std::max<size_t>(sz[b], 16)));
    HIP_TRY(B[11].ensure(std::max<size_t>(sz[10], 16)));
    HIP_TRY(hipMemcpy(B[0].p, qpeq.data(), sz[0], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(B[1].p, qlen.data(), sz[1], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(B[2].p, qidx, sz[2], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(B[3].p, codes.data(), sz[3], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(B[4].p, toff, sz[4], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(B[5].p, k, sz[5], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(B[6].p, mode, sz[6], hipMemcpyHostToDevice));
    int e = smx_launch_align_batch(nullptr, (const unsigned long long *)B[0].p, (const int *)B[1].p, (const unsigned *)B[2].p,
                                   (const unsigned char *)B[3].p, (const unsigned long long *)B[4].p, (const int *)B[5].p,
                                   (const unsigned char *)B[6].p, n, (unsigned char *)B[7].p, (int *)B[8].p, (int *)B[9].p,
                                   (int *)B[10].p, (int *)B[11].p, cap);
    if (e != 0) return fail(SMX_ERR_DEVICE, "alignment kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dist, B[8].p, sz[8], hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(nloc, B[9].p, sz[9], hipMemcpyDeviceToHost));
    if (cap) {
        HIP_TRY(hipMemcpy(starts, B[10].p, sz[10], hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ends, B[11].p, sz[10], hipMemcpyDeviceToHost));
    }
    return SMX_OK;
}

// ---- specimine: batched long-read HW distances (smx_mine.hip); grow-only device workspace, calls serialised
namespace {
std::mutex g_mine_mutex;
DevBuf g_mine_ws[9];    // queries, qoff, targets, target offsets, lengths, pairs, chunk starts, scratch, jobs + output

// per query: LDS bytes of its Peq table ((distinct bytes + 1) x padded words) and the register class of its per-lane state
int mine_queries(const char *queries, const uint64_t *qoff, uint32_t n_queries, std::vector<size_t> *qlds_out,
                 std::vector<int> *qclass_out) {
    std::vector<size_t> &qlds = *qlds_out;
    std::vector<int> &qclass = *qclass_out;
    qlds.assign(n_queries, 0);
    qclass.assign(n_queries, 0);
    for (uint32_t q = 0; q < n_queries; q++) {
        if (qoff[q + 1] <= qoff[q]) return fail(SMX_ERR_ARG, "query %u is empty", q);
        const uint64_t m = qoff[q + 1] - qoff[q];
        if (m > (uint64_t)INT32_MAX) return fail(SMX_ERR_UNSUPPORTED, "query %u: length %llu", q, (unsigned long long)m);
        bool seen[256] = {false};
        int rows = 0;
        for (uint64_t i = qoff[q]; i < qoff[q + 1]; i++) {
            const unsigned char c = (unsigned char)queries[i];
            if (!seen[c]) { seen[c] = true; rows++; }
        }
        const size_t W = (size_t)((m + 63) / 64), Wp = W | 1;
        qlds[q] = (MINE_LDS_HEAD + (size_t)(rows + 1) * Wp) * 8;
        if (qlds[q] > SMX_LDS_POOL)
            return fail(SMX_ERR_UNSUPPORTED, "query %u: %d distinct bytes x %zu words do not fit the LDS (%zu > %zu bytes)", q,
                        rows, W, qlds[q], (size_t)SMX_LDS_POOL);
        qclass[q] = W <= 1 ? 1 : W <= 2 ? 2 : W <= 4 ? 3 : W <= 8 ? 4 : W <= 16 ? 5 : 0;
    }
    return SMX_OK;
}

// targets: 16-byte aligned copies, 16 bytes of slack at the end (the kernel loads 16 bytes at a time)
int mine_targets(const char *targets, const uint64_t *toff, uint32_t n_targets, std::vector<uint64_t> *tdoff_out,
                 std::vector<int32_t> *tlen_out, std::vector<unsigned char> *tpad) {
    std::vector<uint64_t> &tdoff = *tdoff_out;
    std::vector<int32_t> &tlen = *tlen_out;
    tdoff.assign(n_targets, 0);
    tlen.assign(n_targets, 0);
    uint64_t tbytes = 0;
    for (uint32_t t = 0; t < n_targets; t++) {
        if (toff[t + 1] < toff[t] || toff[t + 1] - toff[t] > (uint64_t)INT32_MAX) return fail(SMX_ERR_ARG, "target %u: bad offsets", t);
        tdoff[t] = tbytes;
        tlen[t] = (int32_t)(toff[t + 1] - toff[t]);
        tbytes += ((uint64_t)tlen[t] + 15) & ~(uint64_t)15;
    }
    tbytes += 16;
    tpad->assign(tbytes, 0);
    for (uint32_t t = 0; t < n_targets; t++) memcpy(tpad->data() + tdoff[t], targets + toff[t], (size_t)tlen[t]);
    return SMX_OK;
}

// One smx_mine_* call.  distances: job j's nq x nt distances at out[sum over earlier jobs of nq * nt] (int32); else
// the best identities at out[sum over earlier jobs of nt] (double).  Device and host memory hold the queries, the
// targets, sum(nq) (job, query) pairs and the output: only the distance output grows with sum(nq * nt).
int mine_call(bool distances, const char *queries, const uint64_t *qoff, uint32_t n_queries, const int32_t *k,
              const char *targets, const uint64_t *toff, uint32_t n_targets, const smx_mine_job *jobs, uint32_t n_jobs,
              void *out, float *kernel_ms) {
    if (!out && n_jobs) return fail(SMX_ERR_ARG, "null argument");
    if (!queries || !qoff || !k || !targets || !toff || (n_jobs && !jobs)) return fail(SMX_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> guard(g_mine_mutex);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SMX_ERR_DEVICE, "libsmx has no CPU path: no HIP device");
    std::vector<size_t> qlds;
    std::vector<int> qclass;
    int rc = mine_queries(queries, qoff, n_queries, &qlds, &qclass);
    if (rc != SMX_OK) return rc;
    std::vector<uint64_t> tdoff;
    std::vector<int32_t> tlen;
    std::vector<unsigned char> tpad;
    rc = mine_targets(targets, toff, n_targets, &tdoff, &tlen, &tpad);
    if (rc != SMX_OK) return rc;
    // jobs -> (job, query) pairs with at least one target, grouped by register class, in query order within a class
    // (a workgroup rebuilds the Peq table only when the query changes)
    std::vector<smx::MineJobDev> djobs(n_jobs);
    std::vector<smx::MinePair> pairs[6];
    size_t lds_max[6] = {0, 0, 0, 0, 0, 0};
    int words_max0 = 0;
    uint64_t dist_off = 0, best_off = 0;
    for (uint32_t j = 0; j < n_jobs; j++) {
        const smx_mine_job &J = jobs[j];
        if ((uint64_t)J.q0 + J.nq > n_queries || (uint64_t)J.t0 + J.nt > n_targets)
            return fail(SMX_ERR_ARG, "job %u: query or target range out of bounds", j);
        djobs[j] = smx::MineJobDev{J.q0, J.nq, J.t0, J.nt, dist_off, best_off, J.min_identity};
        dist_off += (uint64_t)J.nq * J.nt;
        best_off += J.nt;
        if (J.nt == 0) continue;
        for (uint32_t i = 0; i < J.nq; i++) {
            const uint32_t q = J.q0 + i;
            const int c = qclass[q];
            lds_max[c] = std::max(lds_max[c], qlds[q]);
            if (c == 0) words_max0 = std::max(words_max0, (int)((qoff[q + 1] - qoff[q] + 63) / 64));
            pairs[c].push_back(smx::MinePair{j, q, k[q], 0});
        }
    }
    const uint64_t n_out = distances ? dist_off : best_off;
    if (n_out == 0) {
        if (kernel_ms) *kernel_ms = 0.0f;
        return SMX_OK;
    }
    const size_t out_bytes = n_out * (distances ? sizeof(int32_t) : sizeof(double));
    size_t npairs = 0;
    std::vector<uint64_t> chunk_start;            // per class: n + 1 prefix entries, one after the other
    uint64_t chunks[6] = {0, 0, 0, 0, 0, 0};
    for (int c = 0; c < 6; c++) {
        std::stable_sort(pairs[c].begin(), pairs[c].end(),
                         [](const smx::MinePair &a, const smx::MinePair &b) { return a.q < b.q; });
        if (pairs[c].empty()) continue;
        chunk_start.push_back(0);
        for (const smx::MinePair &P : pairs[c]) {
            chunks[c] += (djobs[P.job].nt + MINE_THREADS - 1) / MINE_THREADS;
            chunk_start.push_back(chunks[c]);
        }
        npairs += pairs[c].size();
    }
    // a workgroup takes MINE_BLOCK_CHUNKS chunks in a row (more where the grid is capped): the pair search and the
    // Peq build of a query's run of chunks are paid once.  Measured on MI355X: one chunk per
    // workgroup loses 1.5x on runs of cheap (decoy) chunks, runs of 8 lose ~11 % to balance on costly chunks
    constexpr uint64_t MINE_BLOCK_CHUNKS = 8;
    const uint64_t grid_cap = (uint64_t)INT32_MAX;
    // the generic class keeps its per-lane state in a global slice per workgroup: bound its grid to ~256 MiB of it
    const size_t slice = (size_t)3 * words_max0 * MINE_THREADS * 8;
    const uint64_t grid0_cap = std::max<size_t>(1, ((size_t)256 << 20) / std::max<size_t>(slice, 1));
    DevBuf *B = g_mine_ws;
    const size_t sz[5] = {(size_t)qoff[n_queries], ((size_t)n_queries + 1) * 8, tpad.size(), (size_t)n_targets * 8,
                          (size_t)n_targets * 4};
    for (int b = 0; b < 5; b++) HIP_TRY(B[b].ensure(std::max<size_t>(sz[b], 16)));
    HIP_TRY(B[5].ensure(npairs * sizeof(smx::MinePair)));
    HIP_TRY(B[6].ensure(chunk_start.size() * 8));
    if (!pairs[0].empty()) HIP_TRY(B[7].ensure((size_t)std::min(chunks[0], grid0_cap) * slice));
    HIP_TRY(B[8].ensure(n_jobs * sizeof(smx::MineJobDev) + out_bytes));
    HIP_TRY(hipMemcpy(B[0].p, queries, sz[0], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(B[1].p, qoff, sz[1], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(B[2].p, tpad.data(), sz[2], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(B[3].p, tdoff.data(), sz[3], hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(B[4].p, tlen.data(), sz[4], hipMemcpyHostToDevice));
    size_t at = 0;
    for (int c = 0; c < 6; c++) {
        if (!pairs[c].empty())
            HIP_TRY(hipMemcpy((char *)B[5].p + at * sizeof(smx::MinePair), pairs[c].data(),
                              pairs[c].size() * sizeof(smx::MinePair), hipMemcpyHostToDevice));
        at += pairs[c].size();
    }
    HIP_TRY(hipMemcpy(B[6].p, chunk_start.data(), chunk_start.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(B[8].p, djobs.data(), n_jobs * sizeof(smx::MineJobDev), hipMemcpyHostToDevice));
    void *d_out = (char *)B[8].p + n_jobs * sizeof(smx::MineJobDev);
    if (!distances) HIP_TRY(hipMemset(d_out, 0, out_bytes));       // +0.0: "no pair counts"
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (kernel_ms) {
        HIP_TRY(hipEventCreate(&ev[0]));
        HIP_TRY(hipEventCreate(&ev[1]));
        HIP_TRY(hipEventRecord(ev[0], nullptr));
    }
    static const int kWords[6] = {0, 1, 2, 4, 8, 16};
    size_t pat = 0, cat = 0;
    int e = 0;
    for (int c = 0; c < 6 && e == 0; c++) {
        const uint32_t n = (uint32_t)pairs[c].size();
        if (!n) continue;
        const uint64_t cap = c == 0 ? std::min(grid_cap, grid0_cap) : grid_cap;
        const uint64_t per_block = std::max(MINE_BLOCK_CHUNKS, (chunks[c] + cap - 1) / cap);
        const uint64_t grid = (chunks[c] + per_block - 1) / per_block;
        e = smx_launch_mine(nullptr, kWords[c], distances, (const unsigned char *)B[0].p, (const uint64_t *)B[1].p,
                            (const unsigned char *)B[2].p, (const uint64_t *)B[3].p, (const int32_t *)B[4].p,
                            (const char *)B[5].p + pat * sizeof(smx::MinePair), (const uint64_t *)B[6].p + cat, n,
                            B[8].p, (int)grid, per_block, lds_max[c], d_out, (unsigned long long *)B[7].p, words_max0);
        pat += n;
        cat += (size_t)n + 1;
    }
    if (e != 0) return fail(SMX_ERR_DEVICE, "mining kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    if (kernel_ms) {
        HIP_TRY(hipEventRecord(ev[1], nullptr));
        HIP_TRY(hipEventSynchronize(ev[1]));
        HIP_TRY(hipEventElapsedTime(kernel_ms, ev[0], ev[1]));
        (void)hipEventDestroy(ev[0]);
        (void)hipEventDestroy(ev[1]);
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
    return SMX_OK;
}
}  // namespace

int smx_mine_distances(const char *queries, const uint64_t *qoff, uint32_t n_queries, const int32_t *k, const char *targets,
                       const uint64_t *toff, uint32_t n_targets, const smx_mine_job *jobs, uint32_t n_jobs, int32_t *dist,
                       float *kernel_ms) {
    return mine_call(true, queries, qoff, n_queries, k, targets, toff, n_targets, jobs, n_jobs, dist, kernel_ms);
}

int smx_mine_best_identity(const char *queries, const uint64_t *qoff, uint32_t n_queries, const int32_t *k,
                           const char *targets, const uint64_t *toff, uint32_t n_targets, const smx_mine_job *jobs,
                           uint32_t n_jobs, double *best, float *kernel_ms) {
    return mine_call(false, queries, qoff, n_queries, k, targets, toff, n_targets, jobs, n_jobs, best, kernel_ms);
}

// ---- inner scan: every pattern against the whole read, hits on the internal columns (smx_inner.hip)
extern "C" int smx_batch_seq_view(const smx_batch *b, const char **seq, uint32_t *len);   // smx_io.cpp

namespace {
std::mutex g_inner_mutex;
DevBuf g_inner_ws[7];   // bases, read offsets, unit starts, unit reads, records, outputs, pattern tables

struct InnerClass {      // the patterns of one word width, in passes of G
    int w64 = 0, G = 4, npass = 0;
    std::vector<uint32_t> idx;        // pattern indices of the call
    size_t peq_at = 0, tab_at = 0;    // offsets into the table blob: match words; pm, pk, jmap (npass * G ints each)
};

constexpr uint64_t INNER_DEFAULT_BUDGET = (uint64_t)1 << 30;

// The reads are seq[i][0 .. len[i]); with `flat` they also lie back to back from flat (seq[i] = flat + flat_off[i]).
int inner_call(const char *patterns, const uint32_t *poff, uint32_t Q, const int32_t *k, const char *const *seq,
               const uint32_t *len, const uint8_t *flat, uint32_t n_reads, int32_t margin, uint32_t H,
               uint64_t budget, uint8_t *nhit, int8_t *hit_dist, int32_t *hit_end, float *kernel_ms) {
    if (!patterns || !poff || !k) return fail(SMX_ERR_ARG, "null argument");
    if (n_reads && (!seq || !len || !nhit || !hit_dist || !hit_end)) return fail(SMX_ERR_ARG, "null argument");
    if (Q < 1 || Q > INNER_MAX_PATTERNS) return fail(SMX_ERR_ARG, "n_patterns %u outside 1..%d", Q, INNER_MAX_PATTERNS);
    if (H < 1 || H > INNER_MAX_HITS) return fail(SMX_ERR_ARG, "max_hits %u outside 1..%d", H, INNER_MAX_HITS);
    if (margin < 0) return fail(SMX_ERR_ARG, "margin %d is negative", margin);
    std::vector<unsigned long long> peq((size_t)Q * 16);
    std::vector<int> pm(Q);
    InnerClass cls[2];
    cls[1].w64 = 1;
    int lead = 1;
    for (uint32_t j = 0; j < Q; j++) {
        if (poff[j + 1] <= poff[j] || poff[j + 1] - poff[j] > 64)
            return fail(SMX_ERR_ARG, "pattern %u: length outside 1..64", j);
        const int m = (int)(poff[j + 1] - poff[j]);
        if (k[j] < 0 || k[j] >= m) return fail(SMX_ERR_ARG, "pattern %u: threshold %d outside 0..%d", j, k[j], m - 1);
        std::string bad;
        if (!build_peq(patterns + poff[j], m, &peq[(size_t)j * 16], &bad)) return fail(SMX_ERR_ARG, "pattern %u: %s", j, bad.c_str());
        pm[j] = m;
        lead = std::max(lead, m + k[j]);
        cls[m > 32 ? 1 : 0].idx.push_back(j);
    }
    const int PL = smx::inner_piece_len(lead), RW = smx::inner_rec_words((int)H);
    std::lock_guard<std::mutex> guard(g_inner_mutex);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SMX_ERR_DEVICE, "libsmx has no CPU path: no HIP device");
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_reads == 0) return SMX_OK;
    // pattern tables: byte -> code map, then per class the match words [pass][code][G] and pm / pk / jmap
    std::vector<unsigned char> blob(256);
    for (int c = 0; c < 256; c++) blob[c] = (unsigned char)code_of((unsigned char)c);
    for (InnerClass &C : cls) {
        if (C.idx.empty()) continue;
        C.G = C.idx.size() <= 4 ? 4 : 8;
        C.npass = (int)((C.idx.size() + C.G - 1) / C.G);
        const size_t slots = (size_t)C.npass * C.G;
        std::vector<int> tab(3 * slots);
        for (size_t s = 0; s < slots; s++) {
            const bool real = s < C.idx.size();
            tab[s] = real ? pm[C.idx[s]] : 1;
            tab[slots + s] = real ? k[C.idx[s]] : -1;
            tab[2 * slots + s] = real ? (int)C.idx[s] : -1;
        }
        if (C.w64) {
            std::vector<uint64_t> w(slots * 16, 0);
            for (size_t s = 0; s < C.idx.size(); s++)
                for (int c = 0; c < 16; c++) w[((s / C.G) * 16 + c) * C.G + s % C.G] = peq[(size_t)C.idx[s] * 16 + c];
            C.peq_at = blob_add(blob, w);
        } else {
            std::vector<uint32_t> w(slots * 16, 0);
            for (size_t s = 0; s < C.idx.size(); s++)
                for (int c = 0; c < 16; c++) w[((s / C.G) * 16 + c) * C.G + s % C.G] = (uint32_t)peq[(size_t)C.idx[s] * 16 + c];
            C.peq_at = blob_add(blob, w);
        }
        C.tab_at = blob_add(blob, tab);
    }
    DevBuf *B = g_inner_ws;
    HIP_TRY(B[6].ensure(blob.size()));
    HIP_TRY(hipMemcpy(B[6].p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    if (budget == 0) budget = INNER_DEFAULT_BUDGET;
    auto pieces_of = [&](uint32_t n) -> uint64_t {
        return (uint64_t)n > 2 * (uint64_t)margin ? ((uint64_t)n - 2 * (uint64_t)margin + PL - 1) / PL : 0;
    };
    const uint64_t out_per_read = (uint64_t)Q * (1 + 5 * (uint64_t)H);
    struct Events {   // destroyed on every way out of the call
        hipEvent_t ev[2] = {nullptr, nullptr};
        ~Events() {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
        }
    } events;
    hipEvent_t *ev = events.ev;
    if (kernel_ms) {
        HIP_TRY(hipEventCreate(&ev[0]));
        HIP_TRY(hipEventCreate(&ev[1]));
    }
    std::vector<uint64_t> roff;
    std::vector<uint32_t> ustart, unit_read;
    std::vector<unsigned char> stage, out;
    // chunks of whole reads: everything one launch group keeps on the device fits the budget (one read always goes)
    for (uint32_t r0 = 0; r0 < n_reads;) {
        uint64_t bytes = 64, units = 0, nb = 0;
        uint32_t r1 = r0;
        while (r1 < n_reads) {
            if (len[r1] > (uint32_t)INT32_MAX) return fail(SMX_ERR_ARG, "read %u: longer than 2^31 - 1 bases", r1);
            const uint64_t np = pieces_of(len[r1]);
            const uint64_t cost = (uint64_t)len[r1] + 12 + np * (4 + (uint64_t)Q * RW * 4) + out_per_read;
            if (r1 > r0 && (bytes + cost > budget || units + np > 0x7fffffffull)) break;
            bytes += cost;
            units += np;
            nb += len[r1];
            r1++;
        }
        if (units > 0xffffffffull) return fail(SMX_ERR_UNSUPPORTED, "read %u: too many pieces for one launch", r0);
        const uint32_t nr = r1 - r0;
        roff.resize((size_t)nr + 1);
        ustart.resize((size_t)nr + 1);
        unit_read.resize((size_t)units);
        roff[0] = 0;
        ustart[0] = 0;
        for (uint32_t i = 0; i < nr; i++) {
            const uint32_t np = (uint32_t)pieces_of(len[r0 + i]);
            roff[i + 1] = roff[i] + len[r0 + i];
            for (uint32_t p = 0; p < np; p++) unit_read[(size_t)ustart[i] + p] = i;
            ustart[i + 1] = ustart[i] + np;
        }
        const unsigned char *src;
        if (flat) {
            src = (const unsigned char *)seq[r0];
        } else {
            stage.resize((size_t)nb);
            for (uint32_t i = 0; i < nr; i++)
                if (len[r0 + i]) memcpy(stage.data() + roff[i], seq[r0 + i], len[r0 + i]);
            src = stage.data();
        }
        const size_t he_bytes = (size_t)nr * Q * H * 4, hd_bytes = (size_t)nr * Q * H, nh_bytes = (size_t)nr * Q;
        HIP_TRY(B[0].ensure((size_t)nb + 32));
        HIP_TRY(B[1].ensure(roff.size() * 8));
        HIP_TRY(B[2].ensure(ustart.size() * 4));
        HIP_TRY(B[3].ensure(std::max<size_t>(unit_read.size() * 4, 16)));
        HIP_TRY(B[4].ensure(std::max<size_t>((size_t)units * Q * RW * 4, 16)));
        HIP_TRY(B[5].ensure(he_bytes + hd_bytes + nh_bytes));
        if (nb) HIP_TRY(hipMemcpy(B[0].p, src, (size_t)nb, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(B[1].p, roff.data(), roff.size() * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(B[2].p, ustart.data(), ustart.size() * 4, hipMemcpyHostToDevice));
        if (units) HIP_TRY(hipMemcpy(B[3].p, unit_read.data(), unit_read.size() * 4, hipMemcpyHostToDevice));
        smx::InnerArgs A{};
        A.lut = (const unsigned char *)B[6].p;
        A.bases = (const smx::mine_u4 *)B[0].p;
        A.roff = (const uint64_t *)B[1].p;
        A.ustart = (const uint32_t *)B[2].p;
        A.unit_read = (const uint32_t *)B[3].p;
        A.n_units = (uint32_t)units;
        A.Q = (int)Q;
        A.H = (int)H;
        A.margin = margin;
        A.PL = PL;
        A.lead = lead;
        A.recs = (uint32_t *)B[4].p;
        int32_t *d_he = (int32_t *)B[5].p;
        int8_t *d_hd = (int8_t *)B[5].p + he_bytes;
        uint8_t *d_nh = (uint8_t *)B[5].p + he_bytes + hd_bytes;
        if (kernel_ms) HIP_TRY(hipEventRecord(ev[0], nullptr));
        int e = 0;
        for (const InnerClass &C : cls) {
            if (C.idx.empty() || units == 0 || e != 0) continue;
            const size_t slots = (size_t)C.npass * C.G;
            A.peq = (const char *)B[6].p + C.peq_at;
            A.pm = (const int *)((const char *)B[6].p + C.tab_at);
            A.pk = A.pm + slots;
            A.jmap = A.pm + 2 * slots;
            e = smx_launch_inner_scan(nullptr, C.w64, C.G, C.npass, &A);
        }
        if (e == 0) e = smx_launch_inner_merge(nullptr, &A, nr, d_nh, d_hd, d_he);
        if (e != 0) return fail(SMX_ERR_DEVICE, "inner scan launch failed: %s", hipGetErrorString((hipError_t)e));
        if (kernel_ms) {
            float ms = 0.0f;
            HIP_TRY(hipEventRecord(ev[1], nullptr));
            HIP_TRY(hipEventSynchronize(ev[1]));
            HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
            *kernel_ms += ms;
        }
        HIP_TRY(hipDeviceSynchronize());
        out.resize(he_bytes + hd_bytes + nh_bytes);
        HIP_TRY(hipMemcpy(out.data(), B[5].p, out.size(), hipMemcpyDeviceToHost));
        memcpy(hit_end + (size_t)r0 * Q * H, out.data(), he_bytes);
        memcpy(hit_dist + (size_t)r0 * Q * H, out.data() + he_bytes, hd_bytes);
        memcpy(nhit + (size_t)r0 * Q, out.data() + he_bytes + hd_bytes, nh_bytes);
        r0 = r1;
    }
    return SMX_OK;
}
}  // namespace

int smx_inner_scan(const char *patterns, const uint32_t *poff, uint32_t n_patterns, const int32_t *k, const uint8_t *bases,
                   const uint64_t *off, uint32_t n_reads, int32_t margin, uint32_t max_hits, uint64_t budget_bytes,
                   uint8_t *nhit, int8_t *hit_dist, int32_t *hit_end, float *kernel_ms) {
    if (n_reads && (!bases || !off)) return fail(SMX_ERR_ARG, "null argument");
    std::vector<const char *> seq(n_reads);
    std::vector<uint32_t> len(n_reads);
    for (uint32_t i = 0; i < n_reads; i++) {
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > (uint64_t)INT32_MAX) return fail(SMX_ERR_ARG, "read %u: bad offsets", i);
        seq[i] = (const char *)bases + off[i];
        len[i] = (uint32_t)(off[i + 1] - off[i]);
    }
    return inner_call(patterns, poff, n_patterns, k, seq.data(), len.data(), bases, n_reads, margin, max_hits, budget_bytes,
                      nhit, hit_dist, hit_end, kernel_ms);
}

int smx_inner_scan_batch(const smx_batch *batch, const char *patterns, const uint32_t *poff, uint32_t n_patterns,
                         const int32_t *k, int32_t margin, uint32_t max_hits, uint64_t budget_bytes, uint8_t *nhit,
                         int8_t *hit_dist, int32_t *hit_end, float *kernel_ms) {
    if (!batch) return fail(SMX_ERR_ARG, "null argument");
    const uint32_t n_reads = smx_batch_size(batch);
    std::vector<const char *> seq(n_reads);
    std::vector<uint32_t> len(n_reads);
    int rc = smx_batch_seq_view(batch, seq.data(), len.data());
    if (rc != SMX_OK) return rc;
    return inner_call(patterns, poff, n_patterns, k, seq.data(), len.data(), nullptr, n_reads, margin, max_hits, budget_bytes,
                      nhit, hit_dist, hit_end, kernel_ms);
}

// ---- lanes: asynchronous host-buffer path (pinned staging, one stream per lane)
struct smx_lane {
    smx_panel *P = nullptr;
    uint32_t cap = 0, n = 0;
    hipStream_t stream = nullptr;
    // pinned host staging
    uint8_t *h_windows = nullptr;
    int32_t *h_lens = nullptr;
    smx_op *h_ops = nullptr, *h_extra = nullptr;
    uint64_t *h_counts = nullptr;   // counts vector followed by one word holding n_extra
    // device
    uint8_t *d_windows = nullptr;
    uint8_t *d_packed = nullptr;    // 4-bit windows as they arrive over PCIe (smx_lane_submit_packed)
    int32_t *d_lens = nullptr;
    smx_op *d_ops = nullptr, *d_extra = nullptr;
    uint64_t *d_counts = nullptr;   // same layout as h_counts
    bool busy = false;
    // match statistics (smx_lane_attach_stats): allocated at the first attach, kept until the lane goes
    smx_stats *stats = nullptr;
    smx_hit *d_hits = nullptr;      // lean hit dump of the batch in flight
    uint32_t *d_fb = nullptr;       // fallback count, then the indices
    uint32_t *h_fb = nullptr;       // pinned copy of d_fb
    bool counted = false;           // the batch in flight went into the table
    bool fb_valid = false;          // h_fb describes the batch smx_lane_wait retired last
};

// the fallback indices that travel with every batch; smx_lane_fallback fetches the rest (trim-to-empty reads are rare)
static uint32_t lane_fb_sent(const smx_lane *L) { return std::min<uint32_t>(L->cap, 4096u); }

void smx_lane_destroy(smx_lane *L) {
    if (!L) return;
    if (L->stream) {
        (void)hipStreamSynchronize(L->stream);
        if (L->P) stream_release(L->P, L->stream);   // the panel's per-stream slot (launch counters, prescan buffers) is free again
    }
    if (L->h_windows) (void)hipHostFree(L->h_windows);
    if (L->h_lens) (void)hipHostFree(L->h_lens);
    if (L->h_ops) (void)hipHostFree(L->h_ops);
    if (L->h_extra) (void)hipHostFree(L->h_extra);
    if (L->h_counts) (void)hipHostFree(L->h_counts);
    if (L->d_windows) (void)hipFree(L->d_windows);
    if (L->d_packed) (void)hipFree(L->d_packed);
    if (L->d_lens) (void)hipFree(L->d_lens);
    if (L->d_ops) (void)hipFree(L->d_ops);
    if (L->d_extra) (void)hipFree(L->d_extra);
    if (L->d_counts) (void)hipFree(L->d_counts);
    if (L->d_hits) (void)hipFree(L->d_hits);
    if (L->d_fb) (void)hipFree(L->d_fb);
    if (L->h_fb) (void)hipHostFree(L->h_fb);
    if (L->stream) (void)hipStreamDestroy(L->stream);
    delete L;
}

int smx_lane_create(const smx_panel *Pc, uint32_t max_reads, smx_lane **out) {
    smx_panel *P = const_cast<smx_panel *>(Pc);
    if (!P || !out || max_reads == 0) return fail(SMX_ERR_ARG, "null argument");
    int rc = ensure_device(P);
    if (rc) return rc;
    smx_lane *L = new smx_lane();
    L->P = P;
    L->cap = max_reads;
    const size_t wb = (size_t)max_reads * P->hp.wstride, ob = (size_t)max_reads * sizeof(smx_op), cb = (smx_counts_len(P) + 1) * 8;
#define LANE_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { smx_lane_destroy(L); return fail(SMX_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); } } while (0)
    LANE_TRY(hipStreamCreateWithFlags(&L->stream, hipStreamNonBlocking));
    LANE_TRY(hipHostMalloc((void **)&L->h_windows, wb, hipHostMallocDefault));
    LANE_TRY(hipHostMalloc((void **)&L->h_lens, (size_t)max_reads * 4, hipHostMallocDefault));
    LANE_TRY(hipHostMalloc((void **)&L->h_ops, ob, hipHostMallocDefault));
    LANE_TRY(hipHostMalloc((void **)&L->h_extra, ob, hipHostMallocDefault));
    LANE_TRY(hipHostMalloc((void **)&L->h_counts, cb, hipHostMallocDefault));
    LANE_TRY(hipMalloc((void **)&L->d_windows, wb));
    LANE_TRY(hipMalloc((void **)&L->d_packed, (size_t)max_reads * smx_packed_stride_for(P->hp.S)));
    LANE_TRY(hipMalloc((void **)&L->d_lens, (size_t)max_reads * 4));
    LANE_TRY(hipMalloc((void **)&L->d_ops, ob));
    LANE_TRY(hipMalloc((void **)&L->d_extra, ob));
    LANE_TRY(hipMalloc((void **)&L->d_counts, cb));
#undef LANE_TRY
    *out = L;
    return SMX_OK;
}

uint8_t *smx_lane_windows(smx_lane *L) { return L ? L->h_windows : nullptr; }
int32_t *smx_lane_lens(smx_lane *L) { return L ? L->h_lens : nullptr; }

static int lane_submit(smx_lane *L, uint32_t n_reads, bool packed);
int smx_lane_submit(smx_lane *L, uint32_t n_reads) { return lane_submit(L, n_reads, false); }
int smx_lane_submit_packed(smx_lane *L, uint32_t n_reads) { return lane_submit(L, n_reads, true); }

static int lane_submit(smx_lane *L, uint32_t n_reads, bool packed) {
    if (!L) return fail(SMX_ERR_ARG, "null argument");
    if (L->busy) return fail(SMX_ERR_ARG, "lane already has a batch in flight: smx_lane_wait first");
    HIP_TRY(hipSetDevice(L->P->device));   // lanes are driven from reader / writer threads: device selection is per thread
    if (n_reads > L->cap) return fail(SMX_ERR_ARG, "batch of %u reads exceeds the lane capacity %u", n_reads, L->cap);
    smx_panel *P = L->P;
    const size_t ncnt = smx_counts_len(P);
    L->n = n_reads;
    L->counted = false;
    L->fb_valid = false;
    HIP_TRY(hipMemsetAsync(L->d_counts, 0, (ncnt + 1) * 8, L->stream));
    if (n_reads) {
        if (packed) {   // the staging holds 4-bit windows: half the bytes over the link, unpacked into the ASCII layout on the device
            const size_t ps = smx_packed_stride_for(P->hp.S);
            HIP_TRY(hipMemcpyAsync(L->d_packed, L->h_windows, (size_t)n_reads * ps, hipMemcpyHostToDevice, L->stream));
            int ue = smx_launch_unpack_windows(L->stream, L->d_packed, L->d_windows, n_reads, P->hp.S, (int)ps, P->hp.wstride, P->n_cu);
            if (ue != 0) return fail(SMX_ERR_DEVICE, "unpack kernel launch failed: %s", hipGetErrorString((hipError_t)ue));
        } else
            HIP_TRY(hipMemcpyAsync(L->d_windows, L->h_windows, (size_t)n_reads * P->hp.wstride, hipMemcpyHostToDevice, L->stream));
        HIP_TRY(hipMemcpyAsync(L->d_lens, L->h_lens, (size_t)n_reads * 4, hipMemcpyHostToDevice, L->stream));
        int rc = smx_batch_run_device(P, L->stream, L->d_windows, L->d_lens, n_reads, L->d_ops, L->d_extra, L->cap,
                                      (uint32_t *)(L->d_counts + ncnt), L->d_counts, L->stats ? L->d_hits : nullptr, nullptr);
        if (rc) return rc;
        if (L->stats) {   // the batch's rows go into the table behind its demux kernel; only the fallback list comes back
            rc = smx_stats_accumulate_device(L->stats, L->stream, L->d_hits, L->d_ops, n_reads, L->d_fb + 1, L->cap, L->d_fb);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(L->h_fb, L->d_fb, (size_t)(1 + lane_fb_sent(L)) * 4, hipMemcpyDeviceToHost, L->stream));
        }
        HIP_TRY(hipMemcpyAsync(L->h_ops, L->d_ops, (size_t)n_reads * sizeof(smx_op), hipMemcpyDeviceToHost, L->stream));
        // extra records are rare: the count is not known on the host yet, so a fixed small prefix travels with the batch and
        // smx_lane_wait fetches the rest if there is more
        HIP_TRY(hipMemcpyAsync(L->h_extra, L->d_extra, (size_t)std::min<uint32_t>(L->cap, std::max<uint32_t>(4096u, n_reads / 64)) * sizeof(smx_op),
                               hipMemcpyDeviceToHost, L->stream));
    }
    HIP_TRY(hipMemcpyAsync(L->h_counts, L->d_counts, (ncnt + 1) * 8, hipMemcpyDeviceToHost, L->stream));
    if (L->stats) {
        if (n_reads == 0) L->h_fb[0] = 0;   // nothing was enqueued that would write it
        L->counted = true;
    }
    L->busy = true;
    return SMX_OK;
}

int smx_lane_wait(smx_lane *L, const smx_op **ops, const smx_op **extra, uint32_t *n_extra, uint64_t *counts) {
    if (!L || !n_extra || !counts) return fail(SMX_ERR_ARG, "null argument");
    if (!L->busy) return fail(SMX_ERR_ARG, "lane has no batch in flight");
    smx_panel *P = L->P;
    HIP_TRY(hipSetDevice(P->device));
    const size_t ncnt = smx_counts_len(P);
    L->busy = false;
    {
        hipError_t se = hipStreamSynchronize(L->stream);
        if (se != hipSuccess) {
            stream_reset_counters(P, L->stream);
            return fail(SMX_ERR_DEVICE, "lane batch failed: %s", hipGetErrorString(se));
        }
    }
    L->fb_valid = L->counted;   // from here on, whatever this call returns: the batch's rows are in the table
    const uint32_t ne = (uint32_t)L->h_counts[ncnt];
    *n_extra = ne;
    if (L->h_counts[SMX_CNT_TOTAL] != L->n) {
        stream_reset_counters(P, L->stream);
        return fail(SMX_ERR_DEVICE, "demux kernel processed %llu of %u reads (tile queue out of step); counters reset",
                    (unsigned long long)L->h_counts[SMX_CNT_TOTAL], L->n);
    }
    if (ne > L->cap) return fail(SMX_ERR_OVERFLOW, "extra buffer too small: need %u records, have %u", ne, L->cap);
    const uint32_t sent = std::min<uint32_t>(L->cap, std::max<uint32_t>(4096u, L->n / 64));
    if (ne > sent)   // the rest of the extra records
        HIP_TRY(hipMemcpy(L->h_extra + sent, L->d_extra + sent, (size_t)(ne - sent) * sizeof(smx_op), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ncnt; i++) counts[i] += L->h_counts[i];
    if (ops) *ops = L->h_ops;
    if (extra) *extra = L->h_extra;
    if (L->h_counts[SMX_CNT_OVERFLOW])
        return fail(SMX_ERR_OVERFLOW, "%llu read(s) produced more than 65535 write operations", (unsigned long long)L->h_counts[SMX_CNT_OVERFLOW]);
    return SMX_OK;
}

// ---- match statistics (smx_stats.hip, smx_stats_core.h)
struct smx_stats {
    smx_panel *panel = nullptr;
    uint32_t cap = 0;
    uint64_t *d_keys = nullptr, *d_counts = nullptr, *d_dropped = nullptr;   // one allocation: keys, counts, dropped
    uint32_t *d_nfb_own = nullptr;                                         // fallback counter when the caller passes none
};

int smx_launch_stats(const smx::StatsPanel *P, void *stream, const smx_hit *d_hits, const smx_op *d_ops, uint32_t n_reads,
                     uint64_t *d_keys, uint64_t *d_counts, uint32_t cap, uint64_t *d_dropped, uint32_t *d_fallback,
                     uint32_t fallback_cap, uint32_t *d_n_fallback, int max_grid);   // smx_stats.hip

int smx_stats_clear(smx_stats *S, void *stream) {
    if (!S) return fail(SMX_ERR_ARG, "null argument");
    HIP_TRY(hipMemsetAsync(S->d_keys, 0xff, (size_t)S->cap * 8, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(S->d_counts, 0, (size_t)S->cap * 8 + 16, (hipStream_t)stream));
    return SMX_OK;
}

int smx_stats_create(const smx_panel *panel, uint32_t capacity, smx_stats **out) {
    if (!panel || !out) return fail(SMX_ERR_ARG, "null argument");
    smx_panel *P = const_cast<smx_panel *>(panel);
    if (P->hp.NPAIR > 4094 || P->hp.NB > 8190)
        return fail(SMX_ERR_UNSUPPORTED, "statistics keys hold at most 4094 primer pairs and 8190 barcodes (panel: %d, %d)",
                    P->hp.NPAIR, P->hp.NB);
    if (capacity > (1u << 28)) return fail(SMX_ERR_ARG, "statistics table capacity %u is above 2^28 slots", capacity);
    int rc = ensure_device(P);
    if (rc != SMX_OK) return rc;
    uint32_t cap = 8;
    while (cap < capacity) cap <<= 1;
    smx_stats *S = new smx_stats();
    S->panel = P;
    S->cap = cap;
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, (size_t)cap * 16 + 16);
    if (e != hipSuccess) { delete S; return fail(SMX_ERR_DEVICE, "hipMalloc(statistics table): %s", hipGetErrorString(e)); }
    S->d_keys = (uint64_t *)p;
    S->d_counts = S->d_keys + cap;
    S->d_dropped = S->d_counts + cap;
    S->d_nfb_own = (uint32_t *)(S->d_dropped + 1);
    rc = smx_stats_clear(S, nullptr);
    if (rc == SMX_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(SMX_ERR_DEVICE, "clearing the statistics table failed");
    if (rc != SMX_OK) { (void)hipFree(p); delete S; return rc; }
    *out = S;
    return SMX_OK;
}

int smx_lane_attach_stats(smx_lane *L, smx_stats *S) {
    if (!L) return fail(SMX_ERR_ARG, "null argument");
    if (L->busy) return fail(SMX_ERR_ARG, "lane has a batch in flight: smx_lane_wait first");
    if (S && S->panel != L->P) return fail(SMX_ERR_ARG, "the statistics table belongs to another panel");
    if (!S) { L->stats = nullptr; return SMX_OK; }
    HIP_TRY(hipSetDevice(L->P->device));
    {   // first attach: the buffers stay with the lane (a failed attach leaves what it got to smx_lane_destroy)
        const size_t hb = (size_t)L->cap * smx_hits_per_read(L->P) * sizeof(smx_hit), fb = ((size_t)L->cap + 1) * 4;
        hipError_t e = hipSuccess;
        if (!L->d_hits) e = hipMalloc((void **)&L->d_hits, hb);
        if (e == hipSuccess && !L->d_fb) e = hipMalloc((void **)&L->d_fb, fb);
        if (e == hipSuccess && !L->h_fb) e = hipHostMalloc((void **)&L->h_fb, fb, hipHostMallocDefault);
        if (e != hipSuccess) return fail(SMX_ERR_DEVICE, "lane statistics buffers: %s", hipGetErrorString(e));
    }
    // the lane's stream does not wait for other streams: whatever was enqueued on the table before (smx_stats_clear on any
    // stream) is complete before the lane's first batch counts into it
    HIP_TRY(hipDeviceSynchronize());
    L->stats = S;
    return SMX_OK;
}

int smx_lane_fallback(smx_lane *L, const uint32_t **idx, uint32_t *n) {
    if (!L || !idx || !n) return fail(SMX_ERR_ARG, "null argument");
    *idx = nullptr;
    *n = 0;
    if (L->busy || !L->fb_valid) return fail(SMX_ERR_ARG, "no counted batch was retired on this lane since its last submit");
    const uint32_t nf = L->h_fb[0], sent = lane_fb_sent(L);
    if (nf > L->n) return fail(SMX_ERR_DEVICE, "statistics kernel reported %u fallback reads in a batch of %u", nf, L->n);
    if (nf > sent) {   // the rest of the list
        HIP_TRY(hipSetDevice(L->P->device));
        HIP_TRY(hipMemcpy(L->h_fb + 1 + sent, L->d_fb + 1 + sent, (size_t)(nf - sent) * 4, hipMemcpyDeviceToHost));
    }
    *idx = L->h_fb + 1;
    *n = nf;
    return SMX_OK;
}

void smx_stats_destroy(smx_stats *S) {
    if (!S) return;
    if (S->d_keys) (void)hipFree(S->d_keys);
    delete S;
}

int smx_stats_accumulate_device(smx_stats *S, void *stream, const smx_hit *d_hits, const smx_op *d_ops, uint32_t n_reads,
                                uint32_t *d_fallback, uint32_t fallback_cap, uint32_t *d_n_fallback) {
    if (!S || (n_reads && (!d_hits || !d_ops))) return fail(SMX_ERR_ARG, "null argument");
    if (!d_fallback) fallback_cap = 0;
    if (!d_n_fallback) d_n_fallback = S->d_nfb_own;
    HIP_TRY(hipMemsetAsync(d_n_fallback, 0, 4, (hipStream_t)stream));
    const smx::DevPanel &h = S->panel->hp;
    smx::StatsPanel sp;
    sp.NP = h.NP; sp.NPAIR = h.NPAIR; sp.preorient = h.preorient;
    sp.pdir = h.pdir; sp.pair_f = h.pair_f; sp.pair_r = h.pair_r;
    // grid-stride launch of `per_cu` workgroups per CU: fewer, longer workgroups combine more rows on chip before they
    // touch the global table (SMX_STATS_BLOCKS_PER_CU: A/B hook of tools/stats_bench.py)
    int per_cu = 2;   // tools/stats_bench.py --grid-sweep: 1, 2, 4, 8 are within 20% of each other; 2 is best or next to best on c2 and c3
    if (const char *e = getenv("SMX_STATS_BLOCKS_PER_CU")) per_cu = std::max(1, atoi(e));
    const int e = smx_launch_stats(&sp, stream, d_hits, d_ops, n_reads, S->d_keys, S->d_counts, S->cap, S->d_dropped,
                                   d_fallback, fallback_cap, d_n_fallback, std::max(1, S->panel->n_cu) * per_cu);
    if (e != 0) return fail(SMX_ERR_DEVICE, "statistics kernel launch: %s", hipGetErrorString((hipError_t)e));
    return SMX_OK;
}

int smx_stats_read(smx_stats *S, uint64_t *keys, uint64_t *counts, uint32_t cap, uint32_t *n, uint64_t *dropped) {
    if (!S || !n) return fail(SMX_ERR_ARG, "null argument");
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint64_t> h((size_t)S->cap * 2 + 1);
    HIP_TRY(hipMemcpy(h.data(), S->d_keys, h.size() * 8, hipMemcpyDeviceToHost));
    const uint64_t lost = h[(size_t)S->cap * 2];
    if (dropped) *dropped = lost;
    *n = 0;
    if (lost)
        return fail(SMX_ERR_OVERFLOW, "the statistics table (%u slots) is full: %llu increments found no slot; raise the "
                    "capacity (--table-capacity)", S->cap, (unsigned long long)lost);
    uint32_t used = 0;
    for (uint32_t s = 0; s < S->cap; s++) used += h[s] != SMX_STATS_EMPTY;
    *n = used;
    if (used > cap || (used && (!keys || !counts))) return fail(SMX_ERR_ARG, "%u distinct keys do not fit the caller's %u", used, cap);
    uint32_t at = 0;
    for (uint32_t s = 0; s < S->cap; s++)
        if (h[s] != SMX_STATS_EMPTY) { keys[at] = h[s]; counts[at] = h[(size_t)S->cap + s]; at++; }
    return SMX_OK;
}

// ---- RCCL over xGMI: one communicator per process (one process per GPU)
int smx_comm_unique_id(uint8_t id[128]) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId u;
    ncclResult_t r = ncclGetUniqueId(&u);
    if (r != ncclSuccess) return fail(SMX_ERR_DEVICE, "ncclGetUniqueId: %s", ncclGetErrorString(r));
    memcpy(id, &u, 128);
    return SMX_OK;
}

int smx_comm_init(const uint8_t id[128], int n_ranks, int rank, void **comm_out) {
    if (!id || !comm_out) return fail(SMX_ERR_ARG, "null argument");
    ncclUniqueId u;
    memcpy(&u, id, 128);
    ncclComm_t comm;
    ncclResult_t r = ncclCommInitRank(&comm, n_ranks, u, rank);
    if (r != ncclSuccess) return fail(SMX_ERR_DEVICE, "ncclCommInitRank: %s", ncclGetErrorString(r));
    *comm_out = (void *)comm;
    return SMX_OK;
}

int smx_counts_allreduce(uint64_t *d_counts, size_t n, void *comm, void *stream) {
    if (!d_counts || !comm) return fail(SMX_ERR_ARG, "null argument");
    ncclResult_t r = ncclAllReduce(d_counts, d_counts, n, ncclUint64, ncclSum, (ncclComm_t)comm, (hipStream_t)stream);
    if (r != ncclSuccess) return fail(SMX_ERR_DEVICE, "ncclAllReduce: %s", ncclGetErrorString(r));
    return SMX_OK;
}

void smx_comm_destroy(void *comm) {
    if (comm) (void)ncclCommDestroy((ncclComm_t)comm);
}

}  // extern "C"
