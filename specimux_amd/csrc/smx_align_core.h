// smx_align_core.h -- the bit-vector column steps and the window geometry that the demux tile (smx_demux_tile.h), its
// scorer (smx_scorer.h) and the alignment kernels (smx_align.hip) share.  Device code.
#ifndef SMX_ALIGN_CORE_H
#define SMX_ALIGN_CORE_H

namespace smx {

// Myers / Hyyro bit-vector column step.  Bits above the pattern length carry garbage
// that never flows downwards (adds carry upwards, shifts go left), so no masking is needed.
template <typename W, bool PREFIX>
__device__ __forceinline__ void myers_step(W Eq, W &Pv, W &Mv, int &score, int top) {
    W Xv = Eq | Mv;
    W Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    W Ph = Mv | ~(Xh | Pv);
    W Mh = Pv & Xh;
    score += (int)((Ph >> top) & 1) - (int)((Mh >> top) & 1);
    Ph = (Ph << 1) | (W)(PREFIX ? 1 : 0);
    Mh <<= 1;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
}

// HW column step for a 32-bit pattern LEFT-ALIGNED in its word (row m-1 = bit 31; the padding rows below the
// pattern have Eq = 0 and stay inert: Pv = 1, Mv = Ph = Mh = 0), so the score delta is two plain shifts of
// the top bit (one of them arithmetic: -1) and a three-operand add.
__device__ __forceinline__ void myers_step_hw_top(unsigned Eq, unsigned &Pv, unsigned &Mv, int &score) {
    unsigned Xv = Eq | Mv;
    unsigned Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    unsigned Ph = Mv | ~(Xh | Pv);
    unsigned Mh = Pv & Xh;
    score = score + (int)(Ph >> 31) + ((int)Mh >> 31);
    // x + x instead of x << 1: measured on gfx950 (tools/ubench/valu_rate.hip, primer_col.hip) v_add_u32 issues
    // faster than v_lshlrev_b32; the asm keeps LLVM from canonicalising the add back into a shift
    asm("v_add_u32 %0, %1, %1" : "=v"(Ph) : "v"(Ph));
    asm("v_add_u32 %0, %1, %1" : "=v"(Mh) : "v"(Mh));
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
}

// Geometry of one end string q of length L.  The stored window holds
// q[L-Sp : L], Sp = min(S, L); window coordinate j <-> q index j + base.
struct EndGeom {
    int Sp;     // stored window length
    int base;   // q index of window position 0
    int j_lo;   // window position where match_one_end's primer target starts
    int shift;  // reference coordinate = (j - j_lo) + shift
};
__device__ __forceinline__ EndGeom end_geom(int L, int S) {
    EndGeom g;
    g.Sp = L < S ? L : S;
    g.base = L - g.Sp;
    if (L >= S) { g.j_lo = 0; g.shift = L - S; }
    else if (L == S - 1) { g.j_lo = 0; g.shift = 0; }           // start == -1 means 0 (alignment.py:37)
    else { int lo = 2 * L - S; g.j_lo = lo > 0 ? lo : 0; g.shift = L - S; }  // negative slice start wraps
    return g;
}

// Barcode target of align_seq(b_rc, q, k, bstart, L, SHW) (demultiplex.py:787-800) in window coordinates.
struct BcGeom {
    int tj0;     // window position of the first target base (may be >= Sp: empty target)
    int delta;   // reference coordinate of window position j = j + base - delta ... see bc_abs()
    bool pf_same; // prefilter slice sequence[bstart:] is the same string as the alignment target
};
__device__ __forceinline__ BcGeom bc_geom(int L, int base, int bstart) {
    BcGeom b;
    int s_ = (bstart == -1) ? 0 : bstart;
    int lo = s_ < 0 ? (L + s_ > 0 ? L + s_ : 0) : (s_ < L ? s_ : L);
    int plo = bstart < 0 ? (L + bstart > 0 ? L + bstart : 0) : (bstart < L ? bstart : L);
    b.tj0 = lo - base;
    b.delta = lo - s_;      // reference coordinate = q index - delta
    b.pf_same = (plo == lo);
    return b;
}

}  // namespace smx
#endif
