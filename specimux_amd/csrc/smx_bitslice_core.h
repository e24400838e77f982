// smx_bitslice_core.h -- the 5-plane bit-sliced counter that the primer prescan (smx_prescan_core.h) and the barcode scans
// (smx_barcode_core.h) keep their last-row score in.  Host/device code like the headers that use it.
#ifndef SMX_BITSLICE_CORE_H
#define SMX_BITSLICE_CORE_H

#include "smx_hd.h"

namespace smx {

// counter += inc - dec (mod 32) per bit position; inc and dec are DISJOINT masks (a horizontal delta is +1, -1 or 0).
// One ripple serves both: t = the positions whose update still propagates into this plane.  Every such position flips its
// bit; an incrementing one carries on through a one, a decrementing one borrows on through a zero:
//     s_i' = s_i ^ t_i        t_(i+1) = t_i & ~(s_i ^ inc)      (the latter is a single v_bitop3_b32)
// Ten instructions for the five planes, against nineteen for an increment ripple followed by a decrement ripple.
SMX_HD void bs_updown5(unsigned &s0, unsigned &s1, unsigned &s2, unsigned &s3, unsigned &s4, unsigned inc, unsigned dec) {
    unsigned t = inc | dec, n;
    n = t & ~(s0 ^ inc); s0 ^= t; t = n;
    n = t & ~(s1 ^ inc); s1 ^= t; t = n;
    n = t & ~(s2 ^ inc); s2 ^= t; t = n;
    n = t & ~(s3 ^ inc); s3 ^= t; t = n;
    s4 ^= t;
}

}  // namespace smx
#endif
