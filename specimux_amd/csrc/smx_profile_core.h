// smx_profile_core.h -- the per-column and per-run code of the error-profile kernel (smx_profile.hip): what one pileup row
// word of a member adds to the member's counts and to its job's tables, given the draft's code at the column and the
// quality byte of the read base it stands for.  Integers only.
//
// Notation.  The draft has m bases; dc(p) is cons_code of its byte at p (0-3 = A C G T, 4 = any other byte), and
// PROFILE_NO_CODE outside [0, m).  The member's row is w[0..m] (smx_cons_core.h): sym_p = w[p] & 7, L_p = (w[p] >> 3) & 255,
// code_i(p) = (w[p] >> (11 + 3 i)) & 7 for i < min(L_p, 4).
//
// Column classes, p < m:  match  sym <= 3, dc <= 3, sym == dc;   sub  sym <= 3, dc <= 3, sym != dc;   del  sym == 5;
// other  the rest (sym == 4 or dc == 4).  L_p > 0, p <= m, is one insertion event of L_p bases.
//
// Read position.  c_p = (sym_p <= 4 ? 1 : 0) + L_p, word m contributing L_m alone.  The base of column p is read byte
// rp(p) = sum_{q < p} c_q + L_p, the bases inserted before it are the bytes rp(p) - L_p .. rp(p) - 1.  Exact unless some
// L_p is 255, the clipped value: such a member is `clipped` and stays out of the q table, the one table that needs a
// read position.
//
// Runs.  A run is a maximal stretch [s, s + r) of the draft of one code b <= 3.  A member's observed length of it is
// obs = #{p in the run: sym_p == b} + #{(p, i): s <= p <= s + r, i < min(L_p, 4), code_i(p) == b}.  The kernel sums this
// column by column: profile_run_votes is column p's share, the kept inserted bases before p that equal b, the base at p
// itself, and for the run's last column the kept inserted bases of word p + 1.  The neighbouring runs have another code,
// so no inserted base counts twice.
//
// Host/device code like smx_resample_core.h: the kernel and tests/cpu/profile_host.h run the same functions.
#ifndef SMX_PROFILE_CORE_H
#define SMX_PROFILE_CORE_H
#include <stdint.h>

#include "smx_hd.h"
#include "smx.h"   // SMX_PROFILE_*, SMX_CONS_MAX_INS

namespace smx {

// the job tables' offsets within SMX_PROFILE_JOB_WORDS: q[64][3], subst[4][5], ins[6], hp[8][7]
constexpr unsigned PROFILE_Q = 0, PROFILE_Q_WORDS = SMX_PROFILE_Q_BINS * 3;
constexpr unsigned PROFILE_SUBST = PROFILE_Q + PROFILE_Q_WORDS;
constexpr unsigned PROFILE_INS = PROFILE_SUBST + 20;
constexpr unsigned PROFILE_HP = PROFILE_INS + 6;
static_assert(PROFILE_HP + 8 * 7 == SMX_PROFILE_JOB_WORDS, "the four tables fill the job's words");

constexpr unsigned PROFILE_NO_CODE = 5;   // dc outside the draft: equal to no column's code
enum : unsigned { PROFILE_MATCH = 0, PROFILE_SUB = 1, PROFILE_DEL = 2, PROFILE_OTHER = 3, PROFILE_NONE = 4 };

SMX_HD unsigned profile_sym(uint32_t w) { return w & 7u; }
SMX_HD unsigned profile_len(uint32_t w) { return (w >> 3) & 255u; }
SMX_HD unsigned profile_kept(uint32_t w) { const unsigned L = profile_len(w); return L < SMX_CONS_MAX_INS ? L : SMX_CONS_MAX_INS; }
SMX_HD unsigned profile_ins_code(uint32_t w, unsigned i) { const unsigned c = (w >> (11u + 3u * i)) & 7u; return c < 4u ? c : 4u; }

// the class of column p of a draft of m bases; PROFILE_NONE for p >= m (word m and the lanes behind it)
SMX_HD unsigned profile_class(uint32_t w, unsigned dc, uint32_t p, uint32_t m) {
    if (p >= m) return PROFILE_NONE;
    const unsigned s = profile_sym(w);
    if (s == 5u) return PROFILE_DEL;
    if (s > 3u || dc > 3u) return PROFILE_OTHER;
    return s == dc ? PROFILE_MATCH : PROFILE_SUB;
}

// c_p: the read bytes word p stands for; 0 for p > m
SMX_HD uint32_t profile_consumed(uint32_t w, uint32_t p, uint32_t m) {
    if (p > m) return 0u;
    return (p < m && profile_sym(w) <= 4u ? 1u : 0u) + profile_len(w);
}

// the column's entry of subst[dc][symbol], or -1 where it has none (dc == 4, another byte in the member, p >= m)
SMX_HD int profile_subst_index(uint32_t w, unsigned dc, uint32_t p, uint32_t m) {
    const unsigned s = profile_sym(w);
    if (p >= m || dc > 3u || s == 4u || s > 5u) return -1;
    return (int)(PROFILE_SUBST + dc * 5u + (s == 5u ? 4u : s));
}

// what word p <= m adds to ins[6]: a count per kept code, and the bases beyond the kept ones
template <typename Add> SMX_HD void profile_ins(uint32_t w, const Add &add) {
    const unsigned L = profile_len(w), kept = profile_kept(w);
    for (unsigned i = 0; i < kept; i++) add(PROFILE_INS + profile_ins_code(w, i), 1u);
    if (L > kept) add(PROFILE_INS + 5u, L - kept);
}

// the Phred bin of a quality byte as it stands in the file
SMX_HD unsigned profile_bin(unsigned char b) {
    const unsigned q = b < 33u ? 0u : (unsigned)b - 33u;
    return q < SMX_PROFILE_Q_BINS - 1u ? q : SMX_PROFILE_Q_BINS - 1u;
}

// What word p adds to q[64][3], for an unclipped member: the base of a match column, of a sub or other column, and every
// inserted base, each under its own byte's bin.  rp = the read position of the column (see above), qual = the read's
// quality bytes, rlen = their number: a position at or behind rlen, which no right row has, is left out, not read.
template <typename Add>
SMX_HD void profile_q(uint32_t w, unsigned cls, uint32_t rp, const unsigned char *qual, uint32_t rlen, const Add &add) {
    const unsigned L = profile_len(w);
    for (unsigned i = 0; i < L; i++) {
        const uint32_t at = rp - L + i;
        if (at < rlen) add(PROFILE_Q + profile_bin(qual[at]) * 3u + 2u, 1u);
    }
    if ((cls == PROFILE_MATCH || cls == PROFILE_SUB || cls == PROFILE_OTHER) && rp < rlen)
        add(PROFILE_Q + profile_bin(qual[rp]) * 3u + (cls == PROFILE_MATCH ? 0u : 1u), 1u);
}

// Runs: column p < m with dc <= 3 starts a stretch when the column before has another code, and ends a run when the
// column behind has; a stretch of other bytes starts like a run (it ends the run before it) and ends none.
SMX_HD bool profile_starts(unsigned dprev, unsigned dc, uint32_t p, uint32_t m) { return p < m && dc != dprev; }
SMX_HD bool profile_ends_run(unsigned dc, unsigned dnext, uint32_t p, uint32_t m) { return p < m && dc <= 3u && dc != dnext; }

// column p's share of its run's observed length; wn = word p + 1, counted for the run's last column only
SMX_HD uint32_t profile_run_votes(uint32_t w, uint32_t wn, unsigned dc, bool ends, uint32_t p, uint32_t m) {
    if (p >= m || dc > 3u) return 0u;
    uint32_t h = profile_sym(w) == dc ? 1u : 0u;
    const unsigned kept = profile_kept(w), kept_n = ends ? profile_kept(wn) : 0u;
    for (unsigned i = 0; i < kept; i++) h += profile_ins_code(w, i) == dc ? 1u : 0u;
    for (unsigned i = 0; i < kept_n; i++) h += profile_ins_code(wn, i) == dc ? 1u : 0u;
    return h;
}

// The sum of the shares over a column's stretch up to the column, within a batch of 64 columns from b0 on: incl = the
// inclusive prefix sum of the shares at the column, excl_at_start = the exclusive one at the stretch's first column where
// that lies in the batch (start >= b0), open = the stretch's sum over the batches before.
SMX_HD uint32_t profile_stretch_sum(uint32_t incl, uint32_t excl_at_start, uint32_t open, uint32_t start, uint32_t b0) {
    return start >= b0 ? incl - excl_at_start : open + incl;
}

// hp[length class][delta + 3] of a run of r bases observed at obs
SMX_HD unsigned profile_hp_index(uint32_t r, uint32_t obs) {
    const int64_t d = (int64_t)obs - (int64_t)r;
    const int delta = d < -3 ? -3 : d > 3 ? 3 : (int)d;
    return PROFILE_HP + ((r < 8u ? r : 8u) - 1u) * 7u + (unsigned)(delta + 3);
}

}  // namespace smx

#endif  // SMX_PROFILE_CORE_H
