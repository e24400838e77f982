// smx_demux.hip -- the demux kernel's instantiations (smx_demux_tile.h), compiled three times (-DSMX_PART=1 / 2 / 3): each part
// instantiates its rows of SMX_DEMUX_VARIANTS (smx_demux_layout.h) and hands them out through smx_demux_fn_p<part>.
#include "smx_demux_tile.h"
#ifndef SMX_PART
#error "compile with -DSMX_PART=1, 2 or 3 (see the Makefile)"
#endif

#define SMX_ROW_SKIP(W, B, C, S_)
#define SMX_ROW_FN(W, B, C, S_) \
    if (v.wbits == W && v.bsv == B && v.cm == C && v.sp == S_) return (const void *)smx::demux_kernel<smx_w##W, 256, B, C, S_>;
// the kernel of a row of this part (nullptr: the row is not one of them)
#if SMX_PART == 1
extern "C" const void *smx_demux_fn_p1(DemuxVariant v) { SMX_DEMUX_VARIANTS(SMX_ROW_FN, SMX_ROW_SKIP, SMX_ROW_SKIP) return nullptr; }
#elif SMX_PART == 2
extern "C" const void *smx_demux_fn_p2(DemuxVariant v) { SMX_DEMUX_VARIANTS(SMX_ROW_SKIP, SMX_ROW_FN, SMX_ROW_SKIP) return nullptr; }
#else
extern "C" const void *smx_demux_fn_p3(DemuxVariant v) { SMX_DEMUX_VARIANTS(SMX_ROW_SKIP, SMX_ROW_SKIP, SMX_ROW_FN) return nullptr; }
#endif
