// smx_host.h -- what the host files of libsmx.so share (smx_api.cpp, smx_panel.cpp, smx_calls.cpp, smx_lane.cpp): the error
// sink, the HIP plumbing every subsystem needs, and struct smx_panel.  Not installed; no .hip file includes it.
#ifndef SMX_HOST_H
#define SMX_HOST_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "smx.h"
#include "smx_blob.h"       // blob_add
#include "smx_internal.h"

// smx_api.cpp (smx_io.cpp uses it too): set the thread-local message and return `code`
extern "C" int smx_set_error(int code, const char *fmt, ...);
#pragma GCC visibility push(hidden)   // what follows is shared between the host files, not exported
constexpr auto fail = &smx_set_error;

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return fail(SMX_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)
#define SMX_TRY(expr) do { int _rc = (expr); if (_rc != SMX_OK) return _rc; } while (0)   // pass a failed call's status on

// No CPU implementation of the hot path exists: every compute entry point asks this first.  *n_devices: the device count.
inline int require_device(int *n_devices = nullptr) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(SMX_ERR_DEVICE, "libsmx has no CPU path: no HIP device available (%s)", hipGetErrorString(e));
    if (n_devices) *n_devices = n;
    return SMX_OK;
}

// smx_api.cpp: the IUPAC alphabet
bool smx_iupac_eq(unsigned char a, unsigned char b);   // symmetric, NOT transitive; false outside ASCII
int code_of(unsigned char ch);                         // index in smx::kCodeChars, 15 = other
unsigned char complement_of(unsigned char ch);
// bit i of peq[c] = eq(pattern[i], char of code c); code 15 never matches
bool build_peq(const char *pat, int m, unsigned long long *peq16, std::string *bad);

struct DevBuf {   // grow-only device buffer of the host-buffer convenience paths; released by hand (some live in globals)
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {   // at least 16 bytes: an empty table is still a pointer a kernel may be handed
        n = std::max<size_t>(n, 16);
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = n + n / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    hipError_t upload(const void *src, size_t bytes, size_t spare = 0) {   // ensure (with `spare` bytes behind) and copy
        hipError_t e = ensure(bytes + spare);
        return e != hipSuccess || bytes == 0 ? e : hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    }
    template <typename T> hipError_t upload(const std::vector<T> &v) { return upload(v.data(), v.size() * sizeof(T)); }
    template <typename T> T *as() const { return (T *)p; }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// Owning handles: device memory, pinned host memory, a stream.  Each converts to what it holds.
struct NoCopy { NoCopy() = default; NoCopy(const NoCopy &) = delete; NoCopy &operator=(const NoCopy &) = delete; };
template <typename T, hipError_t (*FREE)(void *)>
struct HipMem : NoCopy {
    T *p = nullptr;
    ~HipMem() { if (p) (void)FREE(p); }
    operator T *() const { return p; }
};
template <typename T> struct DevMem : HipMem<T, hipFree> {
    hipError_t alloc(size_t bytes) { return this->p ? hipSuccess : hipMalloc((void **)&this->p, bytes); }
};
template <typename T> struct PinMem : HipMem<T, hipHostFree> {
    hipError_t alloc(size_t bytes) { return this->p ? hipSuccess : hipHostMalloc((void **)&this->p, bytes, hipHostMallocDefault); }
};
struct Stream : NoCopy {
    hipStream_t s = nullptr;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

// Times what a call enqueues on the null stream between start() and stop(), which waits for it.
struct KernelTimer : NoCopy {
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~KernelTimer() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    hipError_t start() {
        for (hipEvent_t &e : ev)   // at the first use
            if (!e) if (hipError_t r = hipEventCreate(&e)) return r;
        return hipEventRecord(ev[0], nullptr);
    }
    hipError_t stop(float *ms) {
        hipError_t r = hipEventRecord(ev[1], nullptr);
        if (r == hipSuccess) r = hipEventSynchronize(ev[1]);
        return r == hipSuccess ? hipEventElapsedTime(ms, ev[0], ev[1]) : r;
    }
};

#define SMX_MAX_STREAMS 16   // distinct streams one panel may be launched on

// The environment switches of a panel: none is needed in production.  This struct is the source of truth (DESIGN.md,
// section 8, has the table); read_switches fills it at every smx_panel_create, and nothing else in smx_panel.cpp looks at the
// environment on a panel's behalf.
struct Switches {
    bool no_prescan = false;         // SMX_NO_PRESCAN: every primer alignment by the demux kernel's scalar scan
    bool prescan_planes = false;     // SMX_PRESCAN_PLANES: the prescan keeps its plane buffer and row-major codes (A/B, parity)
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

using smx::TilePlan;   // one per launch mode; ensure_device fills blocks_per_cu
// lean: no per-barcode slots.  slots: --trim tails where the lean kernel cannot report the extent, parity dumps.  compact:
// tiles of the lean kernel (panels with many primers) that keep per-alignment records only for the nitems alignments the match
// words flag; a tile that needs more goes on the overflow list and is redone by a dense lean launch right behind the compact one.
enum { LEAN, SLOTS, COMPACT, N_MODES };

struct PanelTable { size_t off, slot; };   // a table of the blob: its offset there, and the offset in DevPanel of the pointer to it

struct smx_panel {
    smx::DevPanel hp;                 // scalar fields valid; pointers filled at upload
    std::vector<unsigned char> blob;  // host image of the device allocation
    std::vector<PanelTable> tables;   // what smx_panel_create put in the blob; ensure_device relocates hp's pointers from it
    int use64 = 0;
    Switches sw;
    TilePlan plan[N_MODES];           // plan_tiles
    int nitems = 0;                   // records per compact tile; 0: compact mode off
    // device state (lazy, one device per process)
    DevMem<unsigned char> d_blob;
    int device = -1;
    int n_cu = 0;
    std::mutex ws_mutex;                     // smx_batch_run is serialised per panel (one workspace)
    struct { DevBuf windows, lens, ops, extra, n_extra, counts, hits, bdist; } ws;
    // Launch counters {tile queue head, -, finished workgroups, extra records}, 64 bytes per slot, self re-arming.
    // One slot per stream the panel has been launched on: launches on one stream are ordered, launches on different
    // streams (double-buffered pipelines) each pull tiles from their own queue.
    DevMem<unsigned> d_tile_counter;
    std::mutex tc_mutex;
    std::vector<void *> tc_streams;          // slot -> stream (valid where tc_used)
    std::vector<char> tc_used;               // a lane gives its slot back when it is destroyed: the next new stream reuses it
    // primer prescan (smx_prescan.hip): bit-sliced HW alignment of every primer over both end windows, run in front of
    // the demux kernel, which then only redoes the alignments the prescan cannot take (smx_prescan_core.h)
    bool pre_ok = false;
    smx::PreDesc pre;
    int pre_mr = 24, pre_nx = 0, pre_blocks_t = 1, pre_blocks_d = 8;   // longest primer, degenerate symbols, residency
    size_t pre_lds = 0;                      // staging of the transpose / tile-codes kernel
    bool pre_tile = false;                   // tile codes: one tile-major code buffer feeds the DP and the demux kernel, no planes
    DevBuf pre_planes[SMX_MAX_STREAMS];      // per stream slot: the 2-bit text planes of the batch (read-tile major); unused with tile codes
    DevBuf pre_recs[SMX_MAX_STREAMS];        // per stream slot: [2 * NP][search_len / 16][n_reads rounded up to a tile] flag words
    DevBuf pre_match[SMX_MAX_STREAMS];       // per stream slot: match words [tile][2 * NP][32 groups] (bit = read reaches the threshold)
    DevBuf pre_codes[SMX_MAX_STREAMS];       // per stream slot: 2-bit codes, row-major [read][end][chunk] or (tile codes) [tile][end][chunk][read],
                                             // + one flag byte per read behind them
    int share = 1;      // smx_panel_set_streams: batches the caller keeps in flight on as many streams
    DevBuf ovf[SMX_MAX_STREAMS];             // per stream slot: overflow list, one entry per compact tile
    hipEvent_t kev[4] = {nullptr, nullptr, nullptr, nullptr};   // smx_debug_kernel_times: start, after transpose, after DP, end
    bool kev_on = false, kev_pre = false;
    DevMem<unsigned long long> d_phase;      // SMX_PHASE_TIMING diagnostic
    int phase_grid = 0;
};

// smx_panel.cpp
int ensure_device(smx_panel *P);                            // first use: upload the blob, query the device
void stream_release(smx_panel *P, void *stream);            // a (synchronised) stream goes away: its slot is free
void stream_reset_counters(smx_panel *P, void *stream);     // after a failed launch on a (synchronised) stream
// What the counts `c` of a retired batch of n_reads say, for smx_batch_run and smx_lane_wait alike: the first failure among
// the checks `what` asks for, in this order.  Both callers add `c` to the caller's counts between two calls of it.
//   BATCH_SCORED  every read was scored exactly once; if not, the stream's launch counters are reset
//   BATCH_OPS     no read needed more than 65535 write operations
//   BATCH_EXTRA   the n_extra extra records fit extra_cap
enum { BATCH_SCORED = 1, BATCH_OPS = 2, BATCH_EXTRA = 4 };
int batch_retired(smx_panel *P, void *stream, const uint64_t *c, uint32_t n_reads, uint32_t n_extra,
                            uint32_t extra_cap, int what);

#pragma GCC visibility pop
extern "C" size_t smx_packed_stride_for(int32_t S);   // smx_io.cpp
extern "C" int smx_launch_unpack_windows(void *stream, const uint8_t *d_packed, uint8_t *d_windows, uint32_t n_reads, int S,
                                         int pstride, int wstride, int n_cu);   // smx_pack.hip
#endif
