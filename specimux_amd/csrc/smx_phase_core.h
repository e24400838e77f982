// smx_phase_core.h -- the per-position and per-member code of the variant kernels (smx_phase.hip): which positions of a
// job's vote table are candidate sites and whether they qualify, what a member's row word says at a site, and the four
// counts that link two sites.  Integers only.
//
// A position p of the (m + 1) x SMX_CONS_VOTE_WORDS vote table yields up to two candidates, in this order:
//   kind 1, the insertion site before p: present = the sum of ins[0][0..4], absent = aligned - present; the minor allele
//           is the smaller of the two, `present` on a tie.  Codes: 1 = present, 0 = absent.
//   kind 0, the base site at p < m: over A, C, G, T and deletion (sym[0..3] and sym[5]; sym[4], "other", is ignored) major
//           = most votes, minor = second most, ties to the lower code in both.  Codes as in the row: 0-3, 5.
// A candidate qualifies when n_minor >= min_reads and 1000 * n_minor >= min_permille * aligned.
//
// Host/device code like smx_cons_core.h: the kernels and tests/cpu/phase_sim.cpp run the same functions.
#ifndef SMX_PHASE_CORE_H
#define SMX_PHASE_CORE_H
#include <stdint.h>

#include "smx_hd.h"
#include "smx.h"   // smx_cons_site, SMX_CONS_MAX_SITES, SMX_CONS_VOTE_WORDS

namespace smx {

enum { PHASE_NEITHER = 0, PHASE_MINOR = 1, PHASE_MAJOR = 2 };

SMX_HD bool phase_qualifies(uint32_t n_minor, uint32_t aligned, uint32_t min_reads, uint32_t min_permille) {
    return n_minor >= min_reads && (uint64_t)1000 * n_minor >= (uint64_t)min_permille * aligned;
}

SMX_HD smx_cons_site phase_make_site(uint32_t p, unsigned kind, unsigned major, unsigned minor, uint32_t n_major, uint32_t n_minor) {
    smx_cons_site s;
    s.pos = p;
    s.kind = (uint8_t)kind;
    s.major = (uint8_t)major;
    s.minor = (uint8_t)minor;
    s.pad = 0;
    s.n_major = n_major;
    s.n_minor = n_minor;
    return s;
}

// the insertion site before p, from the position's vote words v[0 .. SMX_CONS_VOTE_WORDS)
SMX_HD smx_cons_site phase_ins_site(const uint32_t *v, uint32_t p, uint32_t aligned) {
    const uint32_t present = v[6] + v[7] + v[8] + v[9] + v[10];
    const uint32_t absent = aligned - present;
    return present <= absent ? phase_make_site(p, 1, 0, 1, absent, present) : phase_make_site(p, 1, 1, 0, present, absent);
}

// the base site at p < m.  Compares over static indices only: the five counts stay in registers.
SMX_HD smx_cons_site phase_base_site(const uint32_t *v, uint32_t p) {
    const uint32_t n[5] = {v[0], v[1], v[2], v[3], v[5]};
    unsigned a = 0;                               // index of the major allele: a strict > keeps the lower code on a tie
    uint32_t na = n[0];
#pragma unroll
    for (unsigned c = 1; c < 5; c++)
        if (n[c] > na) { a = c; na = n[c]; }
    unsigned b = a == 0 ? 1u : 0u;                // the most votes among the rest
    uint32_t nb = a == 0 ? n[1] : n[0];
#pragma unroll
    for (unsigned c = 1; c < 5; c++)
        if (c != a && c != (a == 0 ? 1u : 0u) && n[c] > nb) { b = c; nb = n[c]; }
    return phase_make_site(p, 0, a == 4 ? 5u : a, b == 4 ? 5u : b, na, nb);
}

// what a member's row word at site.pos holds: the site's minor allele, its major allele, or neither
SMX_HD unsigned phase_classify(uint32_t word, unsigned kind, unsigned major, unsigned minor) {
    const unsigned code = kind ? (unsigned)(((word >> 3) & 255u) != 0u) : (word & 7u);
    return code == minor ? PHASE_MINOR : code == major ? PHASE_MAJOR : PHASE_NEITHER;
}

SMX_HD int phase_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}

// What one plane word of two sites s < t adds to link[s][t][0..4): (minor, minor), (minor_s, major_t), (major_s, minor_t),
// (major, major).
SMX_HD void phase_link_word(uint64_t minor_s, uint64_t major_s, uint64_t minor_t, uint64_t major_t, uint32_t (&n)[4]) {
    n[0] += (uint32_t)phase_popc(minor_s & minor_t);
    n[1] += (uint32_t)phase_popc(minor_s & major_t);
    n[2] += (uint32_t)phase_popc(major_s & minor_t);
    n[3] += (uint32_t)phase_popc(major_s & major_t);
}

}  // namespace smx

#endif  // SMX_PHASE_CORE_H
