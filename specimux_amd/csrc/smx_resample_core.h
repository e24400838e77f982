// smx_resample_core.h -- the per-member and per-column code of the resampling kernel (smx_resample.hip): what one pileup
// row word adds to a replicate's counters at a column, and whether the replicate keeps the column, that is whether
// consensus.call_consensus over the replicate's votes would emit there what the draft has.  Integers only.
//
// A replicate is a subset of a job's members; its voters are the members of the subset within their limit.  At column
// p of a draft of m bases the replicate counts, over its voters' row words (smx_cons_core.h): a[0..3] the words whose
// symbol is A, C, G, T; del the deletions; ins the words with an insertion before p (the sum of slot 0's five vote
// counters: a member votes in slot 0 exactly when its insertion is not empty); n the voters.  With dc the code of the
// draft's byte at p, the replicate keeps column p iff
//     !(2 ins > n)  &&  ( p == m  ||  ( !(2 del > n)  &&  ( max a == 0  ||  (dc < 4 && a[dc] == max a) ) ) )
// no insertion slot is emitted before p, the base is not dropped, and the base called is the draft's: the draft's base
// wins a tie it is part of and stands where no voter has A, C, G or T.  Word m carries the insertion test alone.
//
// Host/device code like smx_phase_core.h: the kernel and tests/cpu/resample_sim.cpp run the same functions.
#ifndef SMX_RESAMPLE_CORE_H
#define SMX_RESAMPLE_CORE_H
#include <stdint.h>

#include "smx_hd.h"
#include "smx.h"   // SMX_CONS_REPLICATES, SMX_CONS_MAX_LEVELS

namespace smx {

struct ResampleCount {
    uint32_t a[4], del, ins, n;
};

SMX_HD ResampleCount resample_zero() { return ResampleCount{{0u, 0u, 0u, 0u}, 0u, 0u, 0u}; }

// A replicate's bit of a mask word by plain shifting: what the host builds use for `bit` below.
struct ResampleLane {
    unsigned lane;
    SMX_HD uint32_t operator()(uint64_t mask) const { return (uint32_t)(mask >> lane) & 1u; }
};

// One member's row word w under the member's mask word mw (0 for a member above its limit), for one replicate:
// bit(mask) is that replicate's bit, 0 or 1, of a 64-bit word.  The symbol's count goes to `packed`, eight 4-bit
// counters, one per symbol 0..7: one shifted add, the shift being the same for the whole wave, where a counter of its own
// per symbol costs a compare and a select each.  A nibble holds RESAMPLE_PACK_MAX members: resample_flush moves the
// nibbles to the counters proper before one could overflow.  The symbols 4 (another byte) and 7 (word m) count as a
// voter and nothing else.  Static indices throughout: the counters stay in registers.
constexpr unsigned RESAMPLE_PACK_MAX = 15;

template <typename Bit>
SMX_HD void resample_count(uint32_t w, uint64_t mw, const Bit &bit, uint32_t &packed, ResampleCount &c) {
    const uint32_t b = bit(mw);
    packed += b << ((w & 7u) << 2);
    c.ins += ((w >> 3) & 255u) != 0u ? b : 0u;
    c.n += b;
}

SMX_HD void resample_flush(uint32_t &packed, ResampleCount &c) {
#pragma unroll
    for (unsigned x = 0; x < 4; x++) c.a[x] += (packed >> (4u * x)) & 15u;
    c.del += (packed >> 20) & 15u;
    packed = 0u;
}

// Whether a replicate with these counts keeps the column; dc = cons_code of the draft's byte (any value where `last`),
// last = the column is p == m.  The doubled counts need 33 bits.
SMX_HD bool resample_keeps(const uint32_t (&a)[4], uint32_t del, uint32_t ins, uint32_t n_b, unsigned dc, bool last) {
    if ((uint64_t)2 * ins > n_b) return false;
    if (last) return true;
    if ((uint64_t)2 * del > n_b) return false;
    uint32_t top = a[0];
#pragma unroll
    for (unsigned x = 1; x < 4; x++) top = a[x] > top ? a[x] : top;
    if (top == 0u) return true;
    const uint32_t own = dc == 0u ? a[0] : dc == 1u ? a[1] : dc == 2u ? a[2] : dc == 3u ? a[3] : 0u;   // top > 0: `other` never equals it
    return own == top;
}

}  // namespace smx

#endif  // SMX_RESAMPLE_CORE_H
