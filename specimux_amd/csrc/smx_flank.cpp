// smx_flank.cpp -- the barcode survey's host side (specimux-barcodes): the device table of flank keys a run is counted
// into, and the stand-alone assignment of keys to candidate barcodes.  Kernels: smx_flank.hip, logic: smx_flank_core.h.
#include "smx_host.h"
#include "smx_flank_core.h"
#include "smx_flank_plan.h"

extern "C" int smx_launch_flank_count(const smx::FlankPanel *P, void *stream, const uint8_t *d_windows, int wstride,
                                      const int32_t *d_lens, const smx_hit *d_hits, uint32_t n_reads, uint64_t *d_keys,
                                      uint64_t *d_counts, uint32_t cap, uint64_t *d_dropped, uint64_t *d_counters,
                                      int max_grid);   // smx_flank.hip
extern "C" int smx_launch_flank_assign(void *stream, const uint64_t *d_keys, uint32_t n_keys, const void *d_cmw, const int *d_clen,
                                       const int *d_cidx, const int *d_pstart, int k, int32_t *d_best, int32_t *d_first,
                                       int32_t *d_ntied);

#pragma GCC visibility push(hidden)
struct smx_flank {   // one device allocation, freed with the object: keys, counts, dropped, counters
    smx_panel *panel = nullptr;
    uint32_t cap = 0;
    smx::FlankPanel fp;
    DevMem<uint64_t> d_keys;
    uint64_t *d_counts = nullptr, *d_dropped = nullptr, *d_counters = nullptr;
    size_t tail_words() const { return 1 + (size_t)fp.NP * SMX_FLANK_N_COUNTERS; }   // behind the counts
};
#pragma GCC visibility pop

int smx_flank_clear(smx_flank *F, void *stream) {
    if (!F) return fail(SMX_ERR_ARG, "null argument");
    HIP_TRY(hipMemsetAsync(F->d_keys, 0xff, (size_t)F->cap * 8, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(F->d_counts, 0, ((size_t)F->cap + F->tail_words()) * 8, (hipStream_t)stream));
    return SMX_OK;
}

int smx_flank_create(const smx_panel *panel, uint32_t capacity, smx_flank **out) {
    if (!panel || !out) return fail(SMX_ERR_ARG, "null argument");
    smx_panel *P = const_cast<smx_panel *>(panel);
    const smx::DevPanel &h = P->hp;
    if (h.bmax + h.kidx > SMX_FLANK_MAX_W)
        return fail(SMX_ERR_UNSUPPORTED, "barcode survey: barcode length %d + index distance %d is above %d bases, the most a "
                    "flank key holds", h.bmax, h.kidx, SMX_FLANK_MAX_W);
    const int *bm = nullptr;   // the host image of the per-barcode lengths
    for (const PanelTable &t : P->tables)
        if (t.slot == offsetof(smx::DevPanel, bm)) bm = (const int *)(P->blob.data() + t.off);
    if (!bm) return fail(SMX_ERR_ARG, "barcode survey: the panel holds no table of barcode lengths");
    for (int b = 0; b < h.NB; b++)
        if (bm[b] != h.bmax)
            return fail(SMX_ERR_UNSUPPORTED, "barcode survey: the panel's barcodes are not all %d long (barcode %d has %d "
                        "letters)", h.bmax, b, bm[b]);
    if (capacity > (1u << 28)) return fail(SMX_ERR_ARG, "flank table capacity %u is above 2^28 slots", capacity);
    SMX_TRY(ensure_device(P));
    uint32_t cap = 8;
    while (cap < capacity) cap <<= 1;
    std::unique_ptr<smx_flank> F(new smx_flank());
    F->panel = P;
    F->cap = cap;
    F->fp = {h.NP, h.S, h.bmax, h.kidx};
    hipError_t e = F->d_keys.alloc(((size_t)cap * 2 + F->tail_words()) * 8);
    if (e != hipSuccess) return fail(SMX_ERR_DEVICE, "hipMalloc(flank table): %s", hipGetErrorString(e));
    F->d_counts = F->d_keys + cap;
    F->d_dropped = F->d_counts + cap;
    F->d_counters = F->d_dropped + 1;
    SMX_TRY(smx_flank_clear(F.get(), nullptr));
    if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(SMX_ERR_DEVICE, "clearing the flank table failed");
    *out = F.release();
    return SMX_OK;
}

void smx_flank_destroy(smx_flank *F) { delete F; }

int smx_flank_accumulate_device(smx_flank *F, void *stream, const uint8_t *d_windows, const int32_t *d_lens,
                                const smx_hit *d_hits, uint32_t n_reads) {
    if (!F || (n_reads && (!d_windows || !d_lens || !d_hits))) return fail(SMX_ERR_ARG, "null argument");
    // grid-stride launch of two workgroups per CU: few, long workgroups combine the popular keys on chip before they touch
    // the global table (smx_flank_core.h has the sizing of the LDS table that goes with it)
    const int e = smx_launch_flank_count(&F->fp, stream, d_windows, F->panel->hp.wstride, d_lens, d_hits, n_reads, F->d_keys,
                                         F->d_counts, F->cap, F->d_dropped, F->d_counters, std::max(1, F->panel->n_cu) * 2);
    if (e != 0) return fail(SMX_ERR_DEVICE, "flank count kernel launch: %s", hipGetErrorString((hipError_t)e));
    return SMX_OK;
}

int smx_flank_read(smx_flank *F, uint64_t *keys, uint64_t *counts, uint32_t cap, uint32_t *n, uint64_t *counters,
                   uint64_t *dropped) {
    if (!F || !n) return fail(SMX_ERR_ARG, "null argument");
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint64_t> h((size_t)F->cap * 2 + F->tail_words());
    HIP_TRY(hipMemcpy(h.data(), F->d_keys, h.size() * 8, hipMemcpyDeviceToHost));
    const uint64_t lost = h[(size_t)F->cap * 2];
    if (dropped) *dropped = lost;
    *n = 0;
    if (lost)
        return fail(SMX_ERR_OVERFLOW, "the flank table (%u slots) is full: %llu increments found no slot; raise the "
                    "capacity (--table-capacity)", F->cap, (unsigned long long)lost);
    uint32_t used = 0;
    for (uint32_t s = 0; s < F->cap; s++) used += h[s] != SMX_STATS_EMPTY;
    *n = used;
    if (used > cap || (used && (!keys || !counts))) return fail(SMX_ERR_ARG, "%u distinct keys do not fit the caller's %u", used, cap);
    uint32_t at = 0;
    for (uint32_t s = 0; s < F->cap; s++)
        if (h[s] != SMX_STATS_EMPTY) { keys[at] = h[s]; counts[at] = h[(size_t)F->cap + s]; at++; }
    if (counters) memcpy(counters, &h[(size_t)F->cap * 2 + 1], (F->tail_words() - 1) * 8);
    return SMX_OK;
}

int smx_flank_assign(const uint64_t *keys, uint32_t n_keys, const char *cands, const uint32_t *cand_off,
                     const uint8_t *cand_primer, uint32_t n_cands, int32_t k, int32_t *best, int32_t *first, int32_t *ntied,
                     float *kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.f;
    smx::FlankAssignPlan plan;   // argument checks and the candidates grouped by primer (smx_flank_plan.h)
    std::string why;
    const int rc = smx::flank_assign_plan(keys, n_keys, cands, cand_off, cand_primer, n_cands, k, best && first && ntied, build_peq,
                                          &plan, &why);
    if (rc != SMX_OK) return fail(rc, "%s", why.c_str());
    const std::vector<int> &pstart = plan.pstart, &clen = plan.clen, &cidx = plan.cidx;
    const std::vector<uint32_t> &cmw = plan.cmw;
    if (n_keys == 0) return SMX_OK;
    SMX_TRY(require_device());
    DevMem<uint64_t> d_keys;
    DevMem<uint32_t> d_cmw;
    DevMem<int> d_meta, d_out;   // clen, cidx, pstart; best, first, ntied
    const size_t nc = std::max<uint32_t>(n_cands, 1);
    HIP_TRY(d_keys.alloc((size_t)n_keys * 8));
    HIP_TRY(d_cmw.alloc(nc * 16));
    HIP_TRY(d_meta.alloc((nc * 2 + 65) * 4));
    HIP_TRY(d_out.alloc((size_t)n_keys * 3 * 4));
    HIP_TRY(hipMemcpy(d_keys, keys, (size_t)n_keys * 8, hipMemcpyHostToDevice));
    if (n_cands) {
        HIP_TRY(hipMemcpy(d_cmw, cmw.data(), (size_t)n_cands * 16, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_meta, clen.data(), (size_t)n_cands * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_meta + nc, cidx.data(), (size_t)n_cands * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(d_meta + 2 * nc, pstart.data(), 65 * 4, hipMemcpyHostToDevice));
    KernelTimer timer;
    HIP_TRY(timer.start());
    const int e = smx_launch_flank_assign(nullptr, d_keys, n_keys, d_cmw, d_meta, d_meta + nc, d_meta + 2 * nc, k, d_out,
                                          d_out + n_keys, d_out + 2 * (size_t)n_keys);
    if (e != 0) return fail(SMX_ERR_DEVICE, "flank assign kernel launch: %s", hipGetErrorString((hipError_t)e));
    float ms = 0.f;
    HIP_TRY(timer.stop(&ms));
    if (kernel_ms) *kernel_ms = ms;
    HIP_TRY(hipMemcpy(best, d_out, (size_t)n_keys * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(first, d_out + n_keys, (size_t)n_keys * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ntied, d_out + 2 * (size_t)n_keys, (size_t)n_keys * 4, hipMemcpyDeviceToHost));
    return SMX_OK;
}
