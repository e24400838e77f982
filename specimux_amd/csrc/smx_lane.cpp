// smx_lane.cpp -- lanes (the asynchronous host-buffer path of libsmx.so: pinned staging, one stream per lane) and the
// match-statistics table (smx_stats.hip, smx_stats_core.h) a lane can count its batches into.
#include "smx_host.h"
#include "smx_stats_core.h"

#pragma GCC visibility push(hidden)
// ---- match statistics: one device allocation, freed with the object
struct smx_stats {
    smx_panel *panel = nullptr;
    uint32_t cap = 0;
    DevMem<uint64_t> d_keys;                                    // keys, then counts, dropped and the fallback counter
    uint64_t *d_counts = nullptr, *d_dropped = nullptr;
    uint32_t *d_nfb_own = nullptr;                              // fallback counter when the caller passes none
};

// ---- lanes.  ~smx_lane synchronises the stream and gives its slot back; then the members go, last to first: buffers, stream.
struct smx_lane {
    smx_panel *P = nullptr;
    uint32_t cap = 0, n = 0;
    Stream stream;
    // pinned host staging
    PinMem<uint8_t> h_windows;
    PinMem<int32_t> h_lens;
    PinMem<smx_op> h_ops, h_extra;
    PinMem<uint64_t> h_counts;      // counts vector followed by one word holding n_extra
    // device
    DevMem<uint8_t> d_windows;
    DevMem<uint8_t> d_packed;       // 4-bit windows as they arrive over PCIe (smx_lane_submit_packed)
    DevMem<int32_t> d_lens;
    DevMem<smx_op> d_ops, d_extra;
    DevMem<uint64_t> d_counts;      // same layout as h_counts
    bool busy = false;
    // match statistics (smx_lane_attach_stats): allocated at the first attach, kept until the lane goes
    smx_stats *stats = nullptr;
    DevMem<smx_hit> d_hits;         // lean hit dump of the batch in flight
    DevMem<uint32_t> d_fb;          // fallback count, then the indices
    PinMem<uint32_t> h_fb;          // pinned copy of d_fb
    bool counted = false;           // the batch in flight went into the table
    bool fb_valid = false;          // h_fb describes the batch smx_lane_wait retired last
    ~smx_lane() {
        if (!stream) return;
        (void)hipStreamSynchronize(stream);
        if (P) stream_release(P, stream);   // the panel's per-stream slot (launch counters, prescan buffers) is free again
    }
};

// the fallback indices that travel with every batch; smx_lane_fallback fetches the rest (trim-to-empty reads are rare)
static uint32_t lane_fb_sent(const smx_lane *L) { return std::min<uint32_t>(L->cap, 4096u); }
// extra records are rare, and their count is not known on the host when the copies are enqueued: a fixed small prefix
// travels with a batch of n reads and smx_lane_wait fetches the rest if there is more
static uint32_t lane_extra_sent(const smx_lane *L, uint32_t n) { return std::min<uint32_t>(L->cap, std::max<uint32_t>(4096u, n / 64)); }
#pragma GCC visibility pop

void smx_lane_destroy(smx_lane *L) { delete L; }

int smx_lane_create(const smx_panel *Pc, uint32_t max_reads, smx_lane **out) {
    smx_panel *P = const_cast<smx_panel *>(Pc);
    if (!P || !out || max_reads == 0) return fail(SMX_ERR_ARG, "null argument");
    SMX_TRY(ensure_device(P));
    std::unique_ptr<smx_lane> L(new smx_lane());   // a failed allocation leaves what it got to ~smx_lane
    L->P = P;
    L->cap = max_reads;
    const size_t wb = (size_t)max_reads * P->hp.wstride, ob = (size_t)max_reads * sizeof(smx_op), cb = (smx_counts_len(P) + 1) * 8;
    HIP_TRY(hipStreamCreateWithFlags(&L->stream.s, hipStreamNonBlocking));
    HIP_TRY(L->h_windows.alloc(wb));
    HIP_TRY(L->h_lens.alloc((size_t)max_reads * 4));
    HIP_TRY(L->h_ops.alloc(ob));
    HIP_TRY(L->h_extra.alloc(ob));
    HIP_TRY(L->h_counts.alloc(cb));
    HIP_TRY(L->d_windows.alloc(wb));
    HIP_TRY(L->d_packed.alloc((size_t)max_reads * smx_packed_stride_for(P->hp.S)));
    HIP_TRY(L->d_lens.alloc((size_t)max_reads * 4));
    HIP_TRY(L->d_ops.alloc(ob));
    HIP_TRY(L->d_extra.alloc(ob));
    HIP_TRY(L->d_counts.alloc(cb));
    *out = L.release();
    return SMX_OK;
}

uint8_t *smx_lane_windows(smx_lane *L) { return L ? L->h_windows : nullptr; }
int32_t *smx_lane_lens(smx_lane *L) { return L ? L->h_lens : nullptr; }

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
        SMX_TRY(smx_batch_run_device(P, L->stream, L->d_windows, L->d_lens, n_reads, L->d_ops, L->d_extra, L->cap,
                                     (uint32_t *)(L->d_counts + ncnt), L->d_counts, L->stats ? L->d_hits : nullptr, nullptr));
        if (L->stats) {   // the batch's rows go into the table behind its demux kernel; only the fallback list comes back
            SMX_TRY(smx_stats_accumulate_device(L->stats, L->stream, L->d_hits, L->d_ops, n_reads, L->d_fb + 1, L->cap, L->d_fb));
            HIP_TRY(hipMemcpyAsync(L->h_fb, L->d_fb, (size_t)(1 + lane_fb_sent(L)) * 4, hipMemcpyDeviceToHost, L->stream));
        }
        HIP_TRY(hipMemcpyAsync(L->h_ops, L->d_ops, (size_t)n_reads * sizeof(smx_op), hipMemcpyDeviceToHost, L->stream));
        HIP_TRY(hipMemcpyAsync(L->h_extra, L->d_extra, (size_t)lane_extra_sent(L, n_reads) * sizeof(smx_op), hipMemcpyDeviceToHost, L->stream));
    }
    HIP_TRY(hipMemcpyAsync(L->h_counts, L->d_counts, (ncnt + 1) * 8, hipMemcpyDeviceToHost, L->stream));
    if (L->stats) {
        if (n_reads == 0) L->h_fb[0] = 0;   // nothing was enqueued that would write it
        L->counted = true;
    }
    L->busy = true;
    return SMX_OK;
}
int smx_lane_submit(smx_lane *L, uint32_t n_reads) { return lane_submit(L, n_reads, false); }
int smx_lane_submit_packed(smx_lane *L, uint32_t n_reads) { return lane_submit(L, n_reads, true); }

int smx_lane_wait(smx_lane *L, const smx_op **ops, const smx_op **extra, uint32_t *n_extra, uint64_t *counts) {
    if (!L || !n_extra || !counts) return fail(SMX_ERR_ARG, "null argument");
    if (!L->busy) return fail(SMX_ERR_ARG, "lane has no batch in flight");
    smx_panel *P = L->P;
    HIP_TRY(hipSetDevice(P->device));
    const size_t ncnt = smx_counts_len(P);
    L->busy = false;
    if (hipError_t se = hipStreamSynchronize(L->stream)) {
        stream_reset_counters(P, L->stream);
        return fail(SMX_ERR_DEVICE, "lane batch failed: %s", hipGetErrorString(se));
    }
    L->fb_valid = L->counted;   // from here on, whatever this call returns: the batch's rows are in the table
    const uint32_t ne = (uint32_t)L->h_counts[ncnt];
    *n_extra = ne;
    SMX_TRY(batch_retired(P, L->stream, L->h_counts, L->n, ne, L->cap, BATCH_SCORED | BATCH_EXTRA));
    const uint32_t sent = lane_extra_sent(L, L->n);
    if (ne > sent)   // the rest of the extra records
        HIP_TRY(hipMemcpy(L->h_extra + sent, L->d_extra + sent, (size_t)(ne - sent) * sizeof(smx_op), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ncnt; i++) counts[i] += L->h_counts[i];
    if (ops) *ops = L->h_ops;
    if (extra) *extra = L->h_extra;
    return batch_retired(P, L->stream, L->h_counts, L->n, ne, L->cap, BATCH_OPS);
}

extern "C" int smx_launch_stats(const smx::StatsPanel *P, void *stream, const smx_hit *d_hits, const smx_op *d_ops,
                                uint32_t n_reads, uint64_t *d_keys, uint64_t *d_counts, uint32_t cap, uint64_t *d_dropped,
                                uint32_t *d_fallback, uint32_t fallback_cap, uint32_t *d_n_fallback, int max_grid);   // smx_stats.hip

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
    SMX_TRY(ensure_device(P));
    uint32_t cap = 8;
    while (cap < capacity) cap <<= 1;
    std::unique_ptr<smx_stats> S(new smx_stats());
    S->panel = P;
    S->cap = cap;
    hipError_t e = S->d_keys.alloc((size_t)cap * 16 + 16);
    if (e != hipSuccess) return fail(SMX_ERR_DEVICE, "hipMalloc(statistics table): %s", hipGetErrorString(e));
    S->d_counts = S->d_keys + cap;
    S->d_dropped = S->d_counts + cap;
    S->d_nfb_own = (uint32_t *)(S->d_dropped + 1);
    SMX_TRY(smx_stats_clear(S.get(), nullptr));
    if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(SMX_ERR_DEVICE, "clearing the statistics table failed");
    *out = S.release();
    return SMX_OK;
}

int smx_lane_attach_stats(smx_lane *L, smx_stats *S) {
    if (!L) return fail(SMX_ERR_ARG, "null argument");
    if (L->busy) return fail(SMX_ERR_ARG, "lane has a batch in flight: smx_lane_wait first");
    if (S && S->panel != L->P) return fail(SMX_ERR_ARG, "the statistics table belongs to another panel");
    if (!S) { L->stats = nullptr; return SMX_OK; }
    HIP_TRY(hipSetDevice(L->P->device));
    {   // first attach: the buffers stay with the lane (a failed attach leaves what it got to the lane)
        const size_t hb = (size_t)L->cap * smx_hits_per_read(L->P) * sizeof(smx_hit), fb = ((size_t)L->cap + 1) * 4;
        hipError_t e = L->d_hits.alloc(hb);   // (alloc keeps what is there)
        if (e == hipSuccess) e = L->d_fb.alloc(fb);
        if (e == hipSuccess) e = L->h_fb.alloc(fb);
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

void smx_stats_destroy(smx_stats *S) { delete S; }

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
