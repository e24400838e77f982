// smx_panel.cpp -- the panel of libsmx.so: compilation of a smx_panel_desc into the device blob, the choice of the demux kernel's
// instantiation (demux_variant) and tile plan (plan_tiles), and the launch glue of the demux kernel (smx_launch_demux,
// smx_batch_run_device, smx_batch_run).  Of the kernel's three headers it includes smx_demux_layout.h alone: the tile
// layout, the table of instantiations, and the three smx_demux_fn_p* of smx_demux.hip that hand out their addresses.
#include "smx_host.h"
#include "smx_barcode_core.h"
#include "smx_demux_layout.h"

static Switches read_switches() {
    Switches w;
    auto on = [](const char *name) { return getenv(name) != nullptr; };
    w.no_prescan = on("SMX_NO_PRESCAN"); w.prescan_planes = on("SMX_PRESCAN_PLANES"); w.no_bitslice = on("SMX_NO_BITSLICE"); w.no_table_sharing = on("SMX_NO_TABLE_SHARING");
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

// ------------------------------------------------------------------------------------------------
// Which instantiation of the demux kernel a launch gets, how much LDS, and the launch itself.
// each part of smx_demux.hip knows its rows of SMX_DEMUX_VARIANTS.  nullptr: no such instantiation; every caller turns that
// into an error
static const void *demux_fn(DemuxVariant v) {
    const void *fn = smx_demux_fn_p1(v);
    if (!fn) fn = smx_demux_fn_p2(v);
    return fn ? fn : smx_demux_fn_p3(v);
}
// The variant a launch with these parameters gets (cm: 0 dense, 1 compact, 2 redo).  Slots mode never uses the bit-sliced
// scan.  The default-flags specialisation applies to the k <= 3 lean kernel (not its tails variant, not the redo launch)
// with the tile sizes it is built for.
static DemuxVariant demux_variant(const smx::DevPanel *P, int use64, int use_slots, int cm, int R, int nitems, bool have_prescan) {
    const int bsv = (use_slots || !P->bs_ok) ? 0 : (P->kidx < 4 ? (P->trim == SMX_TRIM_TAILS ? 3 : 1) : 2);
    DemuxVariant v = {use64 ? 64 : 32, bsv, cm, 0};
    const bool flags = have_prescan && !use64 && bsv == 1 && cm != 2 && (cm == 0 || nitems == 256) && !P->cap_hits && !P->cap_ents &&
                       P->kidx == 3 && P->maxB <= 32 && !P->need_starts && P->trim == SMX_TRIM_BARCODES && P->derep == SMX_DEREP_BEST &&
                       P->preorient && P->minlen == -1 && P->maxlen == -1 && !P->dbg_phase && !(P->no_sp & 1);
    if (!flags) return v;
    if (P->S == 160 && R == 32 && cm == 1) v.sp = 3;                       // wide windows, compact 32-read tiles
    else if (P->S == 80 && R == SMX_SP2_R && cm == 0 && P->NP == 2 && P->NPAIR == 1 && !(P->no_sp & 2) && P->tile_codes) v.sp = 2;
    else if (P->S == 80 && R == 64) v.sp = 1;
    return v;
}

static int smx_launch_demux(const smx::DevPanel *P, int use64, int use_slots, const smx::TilePlan *plan, int grid,
                            const smx::DemuxBatch *b, const smx::DemuxAux *aux_in) {
    smx::DemuxAux aux = *aux_in;
    smx::DemuxBatch a = *b;
    int R = plan->R;
    if (aux.nitems > 0 && (use_slots || !a.pre || !aux.match || !aux.ovf_list || aux.nitems > 256)) return (int)hipErrorInvalidValue;
    if (aux.redo && (!aux.ovf_list || aux.Rc < 1)) return (int)hipErrorInvalidValue;
    if ((aux.nitems > 0 || aux.redo) && use64) return (int)hipErrorInvalidValue;   // (the prescan serves primers of <= 31 nt only)
    if (aux.nitems > 0 && !aux.chain) return (int)hipErrorInvalidValue;              // a compact launch needs its redo launch
    if (R > 64) return (int)hipErrorInvalidValue;
    if (aux.codes2 && (aux.tiled != 0) != (P->tile_codes != 0)) return (int)hipErrorInvalidValue;   // (the variant is chosen by the panel's layout)
    // tile_counter = {tile queue head, overflow tiles, finished workgroups, extra records}: zero at allocation, re-armed
    // by the last workgroup of every launch (of the last launch of a chain).
    const void *fn = demux_fn(demux_variant(P, use64, use_slots, aux.nitems > 0 ? 1 : (aux.redo ? 2 : 0), R, aux.nitems,
                                            aux.codes2 != nullptr && a.pre != nullptr));
    if (!fn) return (int)hipErrorInvalidDeviceFunction;
    smx::DevPanel pv = *P;
    unsigned long long *counts = (unsigned long long *)a.counts;
    void *args[] = {&pv, &a.windows, &a.lens, &a.n_reads, &R, &a.ops, &a.extra, &a.extra_cap, &a.n_extra, &counts, &a.hits, &a.bdist,
                    &a.tile_counter, &use_slots, &a.pre, &a.npad, &aux};
    hipError_t e = hipLaunchKernel(fn, dim3(grid), dim3(256), args, plan->lds, (hipStream_t)a.stream);
    return (int)(e != hipSuccess ? e : hipGetLastError());
}

// The layout of a tile of R reads (nitems > 0: a compact tile with that many records) as DemuxTile::setup computes it from the
// same panel: the default-flags kernels are only selected where their constants are the panel's values.
static smx::TileLayout panel_layout(const smx::DevPanel *P, int use64, int R, int slots, int nitems, bool test_caps) {
    const smx::LayoutArgs la = smx::layout_args(P->NP, P->NB, P->n_pbc, P->NPAIR, P->trim);
    auto layout = [&](auto w) {
        return smx::make_layout<decltype(w)>(P->NP, P->NB, P->S, R, P->maxB, P->need_starts, la.npmeta, P->kidx, slots, P->bs_ok,
                                             la.ncand, test_caps ? P->cap_hits : 0, test_caps ? P->cap_ents : 0, nitems, la.tails,
                                             P->n_bstab);
    };
    return use64 ? layout(smx_w64()) : layout(smx_w32());
}

// LDS bytes of a tile of R reads (nitems > 0: a compact tile with that many records).  The test caps only shrink a tile.
static size_t smx_demux_lds_bytes(const smx::DevPanel *P, int use64, int R, int slots, int nitems) {
    return (size_t)panel_layout(P, use64, R, slots, nitems, false).total;
}

// The instantiation row (cm: 0 dense, 1 compact, 2 redo) a launch with these parameters gets and, with sizes != nullptr, the
// MBW, G, CAPH and CAPE of its tile layout (nitems: what the launch passes -- 0 for the dense and redo launches).  For
// plan_tiles and smx_panel_plan.  Nonzero: the library holds no such instantiation.
static int smx_demux_plan_query(const smx::DevPanel *P, int use64, int use_slots, int cm, int R, int nitems, int have_prescan,
                                smx_plan_variant *row, smx_plan_mode *sizes) {
    const DemuxVariant v = demux_variant(P, use64, use_slots, cm, R, nitems, have_prescan != 0);
    *row = {v.wbits, v.bsv, v.cm, v.sp};
    if (sizes) {
        const smx::TileLayout t = panel_layout(P, use64, R, use_slots, nitems, true);
        sizes->MBW = t.MBW; sizes->G = t.G; sizes->CAPH = t.CAPH; sizes->CAPE = t.CAPE;
    }
    return demux_fn(v) ? 0 : 1;
}

static int smx_set_demux_lds_limit(int use64, size_t bytes) {
    hipError_t e = hipSuccess;
#define SMX_ROW_LIMIT(W, B, C, S_)                                                                                       \
    if (W == (use64 ? 64 : 32)) {                                                                                        \
        const void *fn = demux_fn({W, B, C, S_});                                                                        \
        hipError_t r = fn ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) : hipErrorInvalidDeviceFunction; \
        if (r != hipSuccess) e = r;                                                                                      \
    }
    SMX_DEMUX_VARIANTS(SMX_ROW_LIMIT, SMX_ROW_LIMIT, SMX_ROW_LIMIT)
    return (int)e;
}

// resident workgroups per CU of the kernel a launch with these parameters would use (cm: 0 dense, 1 compact, 2 redo)
static int smx_query_occupancy(const smx::DevPanel *P, int use64, int use_slots, int cm, int R, int nitems, size_t lds_bytes,
                               int *blocks_per_cu, int have_prescan) {
    const void *fn = demux_fn(demux_variant(P, use64, use_slots, cm, R, nitems, have_prescan != 0));
    if (!fn) return (int)hipErrorInvalidDeviceFunction;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, fn, 256, lds_bytes);
    // The API divides the CU's 163 840 bytes by the request.  The hardware hands LDS out in 512-byte granules from 159 744
    // bytes (tools/ubench/lds_residency.hip: a 32 256-byte workgroup is resident four times, not five; 54 272 bytes twice,
    // not three times): workgroups the grid counts on but the CU cannot hold would start after the tile queue has drained.
    if (e == hipSuccess && lds_bytes > 0) {
        const int fit = (int)(SMX_LDS_POOL / ((lds_bytes + 511) & ~(size_t)511));
        if (*blocks_per_cu > fit) *blocks_per_cu = fit < 1 ? 1 : fit;
    }
    return (int)e;
}

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
        smx_plan_variant row;
        (void)smx_demux_plan_query(&h, use64, 0, 1, R, items, 1, &row, nullptr);
        if (row.sp != 0) {
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

int smx_panel_create(const smx_panel_desc *d, smx_panel **out) {
    if (!d || !out) return fail(SMX_ERR_ARG, "null argument");
    if (d->abi_version != SMX_ABI_VERSION) return fail(SMX_ERR_ARG, "ABI version mismatch: %u", d->abi_version);
    const int NP = (int)d->n_primers, NB = (int)d->n_barcodes, NS = (int)d->n_specimens, NPAIR = (int)d->n_pairs;
    if (NP <= 0 || NB <= 0 || NS <= 0 || NPAIR <= 0) return fail(SMX_ERR_ARG, "empty panel");
    if (NP > 64) return fail(SMX_ERR_UNSUPPORTED, "more than 64 distinct primers (%d)", NP);
    if (NPAIR > 127) return fail(SMX_ERR_UNSUPPORTED, "more than 127 primer pairs (%d)", NPAIR);
    // the per-barcode ("slots") kernel keeps a Peq table of 64 bytes per barcode in LDS, the count rounded up to a power of
    // two: 4096 slots are 262 144 bytes, more than a CU has.  Up to 2048 the LDS check at the end decides.
    if (NB > 2048) return fail(SMX_ERR_UNSUPPORTED, "more than 2048 distinct barcodes (%d)", NB);
    if (d->search_len < 1 || d->search_len > 256)
        return fail(SMX_ERR_UNSUPPORTED, "search_len %d outside 1..256", d->search_len);
    if (d->k_index < 0 || d->k_index > 32) return fail(SMX_ERR_UNSUPPORTED, "index edit distance %d outside 0..32", d->k_index);
    if (d->trim < 0 || d->trim > 3 || d->dereplicate < 0 || d->dereplicate > 1) return fail(SMX_ERR_ARG, "bad trim/dereplicate");

    std::unique_ptr<smx_panel> owner(new smx_panel());   // every exit below but the last drops it
    smx_panel *P = owner.get();
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
        if (m < 1 || m > 64) return fail(SMX_ERR_UNSUPPORTED, "primer %d has length %d (supported 1..64)", p, m);
        std::string pat(d->primer_rc + a, m), rpat(pat.rbegin(), pat.rend());
        if (!build_peq(pat.data(), m, &ppeq[p * 16], &bad) || !build_peq(rpat.data(), m, &prpeq[p * 16], &bad)) return fail(SMX_ERR_UNSUPPORTED, "primer %d: %s", p, bad.c_str());
        pm[p] = m;
        pk[p] = d->primer_k[p];
        if (pk[p] < 0 || pk[p] >= m) return fail(SMX_ERR_UNSUPPORTED, "primer %d: edit distance %d must be in 0..len-1", p, pk[p]);
        pdir[p] = d->primer_dir[p] ? 1 : 0;
        pfidx[p] = d->primer_file_index[p];
        if (pfidx[p] < 0 || pfidx[p] > 2000) return fail(SMX_ERR_UNSUPPORTED, "primer file index %d outside 0..2000", pfidx[p]);
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
                                            smx_iupac_eq);
        if (P->pre_ok) {
            P->pre_mr = maxm;
            P->pre_nx = P->pre.nsym - 4;
            // Text of the DP kernel: tile codes for panels of at most two primers, where the transpose kernel's bit transposes
            // cost more than the one per (tile, primer, chunk) the DP kernel does instead.  With more primers every primer's
            // wave would repeat the tile's transposes: those panels keep the planes.
            // (every DP instantiation fits its registers on tile codes without scratch: profiles/ab_tile_codes.txt)
            P->pre_tile = NP <= 2 && !sw.prescan_planes;
            P->pre_lds = smx_prescan_lds_bytes(h.S, P->pre_tile);
            if (P->pre_lds > SMX_LDS_POOL) P->pre_ok = false;
        }
    }
    if (maxB > 1024) return fail(SMX_ERR_UNSUPPORTED, "more than 1024 barcodes on one primer (%d)", maxB);
    std::vector<int> pbc(std::max(pbc_off[NP], 1));
    for (int i = 0; i < pbc_off[NP]; i++) {
        pbc[i] = (int)d->primer_bc[i];
        if (pbc[i] < 0 || pbc[i] >= NB) return fail(SMX_ERR_ARG, "primer_bc[%d] out of range", i);
    }
    std::vector<unsigned> bpeq(NB * 16);
    std::vector<int> bm(NB);
    for (int b = 0; b < NB; b++) {
        int a = (int)d->barcode_rc_off[b], m = (int)d->barcode_rc_off[b + 1] - a;
        if (m < 1 || m > 32) return fail(SMX_ERR_UNSUPPORTED, "barcode %d has length %d (supported 1..32)", b, m);
        if (d->k_index >= m) return fail(SMX_ERR_UNSUPPORTED, "index edit distance %d >= barcode length %d", d->k_index, m);
        unsigned long long t[16];
        if (!build_peq(d->barcode_rc + a, m, t, &bad)) return fail(SMX_ERR_UNSUPPORTED, "barcode %d: %s", b, bad.c_str());
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
    h.cap_hits = sw.cap_hits; h.cap_ents = sw.cap_ents; h.no_sp = sw.no_sp; h.tile_codes = P->pre_tile ? 1 : 0;   // the switches the kernel and its glue look at
    h.bs_m = bm[0];
    if (h.pfmin != 0 && h.pfmin < 2) return fail(SMX_ERR_UNSUPPORTED, "prefilter min length %d < 2: disable the prefilter", h.pfmin);
    if (h.bmax + h.kidx > 200) return fail(SMX_ERR_UNSUPPORTED, "barcode length + k too large");
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
        if (pair_f[i] >= NP || pair_r[i] >= NP || pdir[pair_f[i]] != 0 || pdir[pair_r[i]] != 1) return fail(SMX_ERR_ARG, "pair %d is not (forward primer, reverse primer)", i);
    }
    // (b1,b2) -> chain of specimens in file order (Specimens.specimen_for_exact_match walks file order)
    std::vector<int> pairhead((size_t)NB * NB, -1), spec_next(NS, -1), spec_pool(NS), tail((size_t)NB * NB, -1);
    std::vector<unsigned long long> p1m(NS), p2m(NS);
    for (int s = 0; s < NS; s++) {
        unsigned b1 = d->spec_b1[s], b2 = d->spec_b2[s];
        if (b1 >= (unsigned)NB || b2 >= (unsigned)NB) return fail(SMX_ERR_ARG, "specimen %d barcode index out of range", s);
        size_t key = (size_t)b1 * NB + b2;
        if (pairhead[key] < 0) pairhead[key] = s; else spec_next[tail[key]] = s;
        tail[key] = s;
        p1m[s] = d->spec_p1mask[s];
        p2m[s] = d->spec_p2mask[s];
        spec_pool[s] = d->spec_pool[s];
    }
    // every table goes into the blob with a note of the DevPanel pointer that is its: ensure_device points it at the device copy
    auto add = [&](auto smx::DevPanel::*field, const auto &v) {
        static_assert(sizeof(*(h.*field)) == sizeof(v[0]), "table and pointer of different element types");
        P->tables.push_back({blob_add(P->blob, v), (size_t)((char *)&(h.*field) - (char *)&h)});
    };
    using DP = smx::DevPanel;
    add(&DP::ppeq, ppeq); add(&DP::prpeq, prpeq); add(&DP::bpeq, bpeq); add(&DP::lut, lut);
    add(&DP::pm, pm); add(&DP::pk, pk); add(&DP::pdir, pdir); add(&DP::pfidx, pfidx);
    add(&DP::pbc_off, pbc_off); add(&DP::pbc, pbc); add(&DP::bm, bm);
    add(&DP::pair_f, pair_f); add(&DP::pair_r, pair_r); add(&DP::pair_pool, pair_pool);
    {   // packed lookup tables (32 bytes per barcode pair)
        std::vector<smx::SpecRec> specrec(NS), pairrec((size_t)NB * NB);
        for (int s2 = 0; s2 < NS; s2++) specrec[s2] = {p1m[s2], p2m[s2], s2, spec_next[s2], spec_pool[s2], 0};
        for (size_t k2 = 0; k2 < pairrec.size(); k2++)
            pairrec[k2] = pairhead[k2] >= 0 ? specrec[pairhead[k2]] : smx::SpecRec{0ull, 0ull, -1, -1, -1, 0};
        add(&DP::pairrec, pairrec); add(&DP::specrec, specrec);
    }
    add(&DP::bs_re, bsre);
    add(&DP::bs_tab, bs_tab);

    P->use64 = maxm > 32 ? 1 : 0;
    plan_tiles(h, P->use64, P->pre_ok, sw, P->plan, &P->nitems);
    // Every plan the panel can launch fits the pool, or the panel is refused as a whole: a panel that ran until the first
    // --trim tails or d_bdist launch would be the worse surprise ("The admitted envelope").
    static const char *const mode_name[N_MODES] = {"lean", "slots", "compact"};
    for (int m = 0; m < N_MODES; m++)
        if (P->plan[m].lds > SMX_LDS_POOL)
            return fail(SMX_ERR_UNSUPPORTED, "the %s tiles of %d read(s) (%d primers, %d barcodes, %d on one primer) do not fit the LDS (%zu > %zu bytes)",
                        mode_name[m], P->plan[m].R, NP, NB, maxB, P->plan[m].lds, SMX_LDS_POOL);
    *out = owner.release();
    return SMX_OK;
}

int smx_panel_plan(const smx_panel *P, smx_plan_info *out) {
    if (!P || !out) return fail(SMX_ERR_ARG, "null argument");
    memset(out, 0, sizeof(*out));
    out->lds_pool = (uint32_t)SMX_LDS_POOL;
    out->nitems = P->nitems; out->use64 = P->use64; out->bs_ok = P->hp.bs_ok;
    out->pre_ok = P->pre_ok ? 1 : 0; out->pre_tile = P->pre_tile ? 1 : 0;
    smx_plan_mode *const modes[N_MODES] = {&out->lean, &out->slots, &out->compact};
    for (int m = 0; m < N_MODES; m++) {
        if (m == COMPACT && P->nitems == 0) continue;
        const TilePlan &t = P->plan[m];
        const int items = m == COMPACT ? P->nitems : 0;
        modes[m]->R = t.R; modes[m]->lds_bytes = (uint32_t)t.lds;
        for (int pre = m == COMPACT ? 1 : 0; pre < 2; pre++)
            if (smx_demux_plan_query(&P->hp, P->use64, m == SLOTS, m == COMPACT, t.R, items, pre, &modes[m]->variant[pre], modes[m]) != 0)
                return fail(SMX_ERR_UNSUPPORTED, "no instantiation of the demux kernel for the %s launch", m == SLOTS ? "slots" : m == COMPACT ? "compact" : "lean");
    }
    if (P->nitems > 0)
        for (int pre = 0; pre < 2; pre++)
            if (smx_demux_plan_query(&P->hp, P->use64, 0, 2, P->plan[LEAN].R, 0, pre, &out->redo[pre], nullptr) != 0)
                return fail(SMX_ERR_UNSUPPORTED, "no instantiation of the demux kernel for the redo launch");
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
    }
    for (DevBuf *b : {&P->ws.windows, &P->ws.lens, &P->ws.ops, &P->ws.extra, &P->ws.n_extra, &P->ws.counts, &P->ws.hits, &P->ws.bdist})
        b->release();
    for (int i = 0; i < SMX_MAX_STREAMS; i++)
        for (DevBuf *b : {&P->pre_recs[i], &P->pre_match[i], &P->pre_codes[i], &P->ovf[i], &P->pre_planes[i]}) b->release();
    for (auto &e : P->kev) if (e) (void)hipEventDestroy(e);
    delete P;
}

size_t smx_counts_len(const smx_panel *P) { return P ? (size_t)SMX_CNT_SPECIMEN0 + P->hp.NS : 0; }
size_t smx_window_stride(const smx_panel *P) { return P ? (size_t)P->hp.wstride : 0; }
size_t smx_packed_stride(const smx_panel *P) { return P ? smx_packed_stride_for(P->hp.S) : 0; }
size_t smx_hits_per_read(const smx_panel *P) { return P ? (size_t)2 * P->hp.NP : 0; }
size_t smx_bdist_per_read(const smx_panel *P) { return P ? (size_t)2 * P->hp.NP * P->hp.maxB : 0; }

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
void stream_release(smx_panel *P, void *stream) {
    std::lock_guard<std::mutex> g(P->tc_mutex);
    for (size_t i = 0; i < P->tc_streams.size(); i++)
        if (P->tc_used[i] && P->tc_streams[i] == stream) P->tc_used[i] = 0;
}

// After a failed or out-of-step launch on `stream` (already synchronised): re-arm THAT stream's launch counters only.
// Other lanes of the panel may have kernels in flight on their own slots.
void stream_reset_counters(smx_panel *P, void *stream) {
    const int sl = stream_slot(P, stream, false);
    if (sl >= 0 && P->d_tile_counter) (void)hipMemset(P->d_tile_counter + 16 * sl, 0, 64);
}

int ensure_device(smx_panel *P) {
    if (P->d_blob) return SMX_OK;
    SMX_TRY(require_device());
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    P->device = dev;
    P->n_cu = prop.multiProcessorCount;
    HIP_TRY(P->d_blob.alloc(P->blob.size()));
    HIP_TRY(hipMemcpy(P->d_blob, P->blob.data(), P->blob.size(), hipMemcpyHostToDevice));
    HIP_TRY(P->d_tile_counter.alloc(64 * SMX_MAX_STREAMS));
    HIP_TRY(hipMemset(P->d_tile_counter, 0, 64 * SMX_MAX_STREAMS));   // the kernel re-arms these counters itself after every launch
    smx::DevPanel &h = P->hp;
    for (const PanelTable &t : P->tables) {   // (every pointer of DevPanel is a plain object pointer: one representation)
        const unsigned char *at = P->d_blob + t.off;
        memcpy((char *)&h + t.slot, &at, sizeof(at));
    }
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
        // (the tile-codes kernel stages 2 * S / 16 rows of 1040 bytes: 34 KB at the largest search_len, 256 -- below the 64 KB that
        // need no attribute; should that limit ever grow, this is where its attribute would be raised too)
        static_assert((2 * (256 / 16) * smx::PRE_TS + smx::PRE_SUBG * 32) * 4 <= 64 * 1024, "tile-codes staging at search_len 256");
        if (!P->pre_tile && P->pre_lds > 64 * 1024 && smx_prescan_set_lds_limit(P->pre_lds) != 0)
            return fail(SMX_ERR_DEVICE, "cannot raise the prescan kernel's dynamic LDS limit to %zu bytes", P->pre_lds);
        int occ_t = 0, occ_d = 0;
        if (smx_prescan_occupancy(P->hp.S, P->pre_mr, P->pre_nx, P->pre_tile, P->pre_lds, &occ_t, &occ_d) != 0 || occ_t < 1 || occ_d < 1) { occ_t = 1; occ_d = 8; }
        P->pre_blocks_t = occ_t;
        P->pre_blocks_d = occ_d;
        if (P->sw.debug) fprintf(stderr, "[smx] prescan (%s): transpose %d workgroups/CU (lds %zu), DP %d waves/CU\n", P->pre_tile ? "tile codes" : "planes", occ_t, P->pre_lds, occ_d);
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
        HIP_TRY(P->d_phase.alloc((size_t)P->phase_grid * 16 * 8));
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
    SMX_TRY(ensure_device(P));
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
        const size_t need_planes = P->pre_tile ? 0 : (size_t)(npad / smx::PRE_TILE) * (P->hp.S >> 4) * 8 * 64 * 4 * sizeof(unsigned);
        const size_t need_match = P->nitems > 0 ? (size_t)(npad / smx::PRE_TILE) * 2 * P->hp.NP * smx::PRE_G * sizeof(unsigned) : 0;
        const size_t need_ovf = compact ? ((size_t)n_reads / comp.R + 2) * sizeof(unsigned) : 0;
        DevBuf &pc = P->pre_codes[slot];
        const size_t codes_bytes = (size_t)npad * 2 * (P->hp.S >> 4) * sizeof(unsigned);   // 2-bit codes, then the flag bytes
        const size_t need_codes = codes_bytes + npad;
        if (need > pb.cap || need_planes > pp.cap || need_match > pm.cap || need_ovf > ov.cap || need_codes > pc.cap) {
            if (pb.p || pp.p) (void)hipStreamSynchronize((hipStream_t)stream);   // earlier launches on this stream still use them
            hipError_t pe = pb.ensure(need);
            if (pe == hipSuccess && need_planes) pe = pp.ensure(need_planes);
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
                                    P->hp.wstride, P->pre_tile ? nullptr : (unsigned *)pp.p, (unsigned *)pb.p, P->nitems > 0 ? (unsigned *)pm.p : nullptr,
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
    const int tiled = P->pre_tile ? 1 : 0;
    int e;
    if (compact) {
        // compact launch over all reads, then the dense launch over the reads of the tiles it put on the overflow list
        // (usually none: its workgroups find an empty list and leave)
        e = launch(comp, grid_of(comp), {(const unsigned *)P->pre_match[slot].p, (unsigned *)P->ovf[slot].p, P->nitems, 0, comp.R, 1, d_codes2, d_naflag, tiled});
        if (e == 0 && P->sw.debug_overflow) {   // diagnostic: how many compact tiles went on the overflow list
            unsigned n_ovf = 0;
            (void)hipMemcpyAsync(&n_ovf, tc + 1, sizeof(unsigned), hipMemcpyDeviceToHost, (hipStream_t)stream);
            (void)hipStreamSynchronize((hipStream_t)stream);
            // (tests read the two numbers from this line: tests/test_panel_limits_gpu.py, tests/test_gpu_parity.py)
            fprintf(stderr, "[smx] compact launch: %u of %u tiles left to the redo launch\n", n_ovf, (n_reads + comp.R - 1) / comp.R);
        }
        // the redo launch usually finds an empty list: one workgroup per CU is enough to start with (its workgroups
        // loop over the list), and an empty 256-workgroup launch costs less than an empty full-residency one
        if (e == 0) e = launch(dense, std::min(grid_of(dense), P->n_cu), {nullptr, (unsigned *)P->ovf[slot].p, 0, 1, comp.R, 0, d_codes2, d_naflag, tiled});
    } else {
        e = launch(dense, grid_of(dense), {nullptr, nullptr, 0, 0, 0, 0, d_codes2, d_naflag, tiled});
    }
    if (e != 0) return fail(SMX_ERR_DEVICE, "demux kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    if (P->kev_on) (void)hipEventRecord(P->kev[3], (hipStream_t)stream);
    return SMX_OK;
}

int smx_unpack_windows_device(const smx_panel *Pc, void *stream, const uint8_t *d_packed, uint32_t n_reads, uint8_t *d_windows) {
    smx_panel *P = const_cast<smx_panel *>(Pc);
    if (!P || !d_packed || !d_windows) return fail(SMX_ERR_ARG, "null argument");
    if (((uintptr_t)d_packed & 3) != 0 || ((uintptr_t)d_windows & 15) != 0) return fail(SMX_ERR_ARG, "window buffers must be 16-byte aligned");
    SMX_TRY(ensure_device(P));
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
        SMX_TRY(ensure_device(P));
        for (auto &e : P->kev) HIP_TRY(hipEventCreate(&e));
    }
    P->kev_on = enable != 0;
    return SMX_OK;
}

int batch_retired(smx_panel *P, void *stream, const uint64_t *c, uint32_t n_reads, uint32_t n_extra, uint32_t extra_cap, int what) {
    if ((what & BATCH_SCORED) && c[SMX_CNT_TOTAL] != n_reads) {
        // every read is counted exactly once by the tile that scored it: anything else means tiles were skipped or
        // repeated (a tile queue that did not start at zero) and the batch's records cannot be trusted
        stream_reset_counters(P, stream);
        return fail(SMX_ERR_DEVICE, "demux kernel processed %llu of %u reads (tile queue out of step); counters reset",
                    (unsigned long long)c[SMX_CNT_TOTAL], n_reads);
    }
    if ((what & BATCH_OPS) && c[SMX_CNT_OVERFLOW])
        return fail(SMX_ERR_OVERFLOW, "%llu read(s) produced more than 65535 write operations", (unsigned long long)c[SMX_CNT_OVERFLOW]);
    if ((what & BATCH_EXTRA) && n_extra > extra_cap)
        return fail(SMX_ERR_OVERFLOW, "extra buffer too small: need %u records, have %u", n_extra, extra_cap);
    return SMX_OK;
}

int smx_batch_run(const smx_panel *Pc, const uint8_t *windows, const int32_t *lens, uint32_t n_reads, smx_op *ops,
                  smx_op *extra, uint32_t extra_cap, uint32_t *n_extra, uint64_t *counts, smx_hit *hits, int8_t *bdist) {
    smx_panel *P = const_cast<smx_panel *>(Pc);
    if (!P || !windows || !lens || !ops || !n_extra || !counts) return fail(SMX_ERR_ARG, "null argument");
    SMX_TRY(ensure_device(P));
    *n_extra = 0;
    if (n_reads == 0) return SMX_OK;
    const size_t wbytes = (size_t)n_reads * P->hp.wstride, ncnt = smx_counts_len(P);
    const size_t hbytes = hits ? (size_t)n_reads * smx_hits_per_read(P) * sizeof(smx_hit) : 0;
    const size_t bbytes = bdist ? (size_t)n_reads * smx_bdist_per_read(P) : 0;
    std::lock_guard<std::mutex> guard(P->ws_mutex);
    auto &W = P->ws;
    HIP_TRY(W.windows.upload(windows, wbytes));
    HIP_TRY(W.lens.upload(lens, (size_t)n_reads * 4));
    HIP_TRY(W.ops.ensure((size_t)n_reads * sizeof(smx_op)));
    HIP_TRY(W.extra.ensure(std::max<size_t>((size_t)extra_cap * sizeof(smx_op), 32)));
    HIP_TRY(W.n_extra.ensure(16));
    HIP_TRY(W.counts.ensure(ncnt * 8));
    if (hits) HIP_TRY(W.hits.ensure(hbytes));
    if (bdist) HIP_TRY(W.bdist.ensure(bbytes));
    HIP_TRY(hipMemset(W.n_extra.p, 0, 16));
    HIP_TRY(hipMemset(W.counts.p, 0, ncnt * 8));
    SMX_TRY(smx_batch_run_device(P, nullptr, W.windows.as<uint8_t>(), W.lens.as<int32_t>(), n_reads, W.ops.as<smx_op>(),
                                 W.extra.as<smx_op>(), extra_cap, W.n_extra.as<uint32_t>(), W.counts.as<uint64_t>(),
                                 hits ? W.hits.as<smx_hit>() : nullptr, bdist ? W.bdist.as<int8_t>() : nullptr));
    if (hipError_t se = hipDeviceSynchronize()) {   // an aborted launch leaves the self re-arming counters in an unknown state
        stream_reset_counters(P, nullptr);
        return fail(SMX_ERR_DEVICE, "demux kernel failed: %s", hipGetErrorString(se));
    }
    std::vector<uint64_t> c(ncnt);
    HIP_TRY(hipMemcpy(ops, W.ops.p, (size_t)n_reads * sizeof(smx_op), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(n_extra, W.n_extra.p, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c.data(), W.counts.p, ncnt * 8, hipMemcpyDeviceToHost));
    if (extra && extra_cap)
        HIP_TRY(hipMemcpy(extra, W.extra.p, (size_t)std::min<uint32_t>(*n_extra, extra_cap) * sizeof(smx_op), hipMemcpyDeviceToHost));
    if (hits) HIP_TRY(hipMemcpy(hits, W.hits.p, hbytes, hipMemcpyDeviceToHost));
    if (bdist) HIP_TRY(hipMemcpy(bdist, W.bdist.p, bbytes, hipMemcpyDeviceToHost));
    SMX_TRY(batch_retired(P, nullptr, c.data(), n_reads, *n_extra, extra_cap, BATCH_SCORED));
    for (size_t i = 0; i < ncnt; i++) counts[i] += c[i];
    return batch_retired(P, nullptr, c.data(), n_reads, *n_extra, extra_cap, BATCH_OPS | BATCH_EXTRA);
}
