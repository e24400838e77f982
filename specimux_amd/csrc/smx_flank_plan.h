// smx_flank_plan.h -- the host-side plan of one smx_flank_assign call (smx_flank.cpp): the argument checks, and the
// candidates regrouped by primer as flank_assign_kernel (smx_flank.hip) reads them -- pstart, and per grouped slot the four
// match words, the length and the caller's index.  Host only and free of HIP calls, so that the CPU simulation
// (tests/cpu/flank_sim.cpp, mode plan) and the sanitizer driver (tests/asan/flank_driver.cpp) run it as it is.  The IUPAC
// alphabet lives in smx_api.cpp, which is not: the plan takes its build_peq as a function.
#ifndef SMX_FLANK_PLAN_H
#define SMX_FLANK_PLAN_H
#include <cstdio>
#include <string>
#include <vector>

#include "smx_flank_core.h"

namespace smx {

constexpr int FLANK_MAX_PRIMERS = 64;   // the primer field of a key is 6 bits wide

// false: a letter outside the alphabet, *bad says which
typedef bool (*FlankBuildPeq)(const char *pat, int m, unsigned long long *peq16, std::string *bad);

struct FlankAssignPlan {
    std::vector<int> pstart;      // 65 entries: the candidates of primer p are the slots [pstart[p], pstart[p + 1])
    std::vector<int> clen, cidx;  // per slot: the candidate's length, its index in the caller's order (ascending in a group)
    std::vector<uint32_t> cmw;    // per slot: the match words for the flank letters A C G T
};

// The plan of a call.  have_out: best, first and ntied are all there.  Returns SMX_OK, or SMX_ERR_ARG and why.
inline int flank_assign_plan(const uint64_t *keys, uint32_t n_keys, const char *cands, const uint32_t *cand_off,
                             const uint8_t *cand_primer, uint32_t n_cands, int32_t k, bool have_out, FlankBuildPeq build_peq,
                             FlankAssignPlan *plan, std::string *why) {
    FlankAssignPlan &P = *plan;
    P = FlankAssignPlan();
    char msg[160];
    if ((n_keys && (!keys || !have_out)) || !cand_off || (n_cands && (!cands || !cand_primer))) {
        *why = "null argument";
        return SMX_ERR_ARG;
    }
    if (k < 0) {
        *why = "negative distance threshold " + std::to_string(k);
        return SMX_ERR_ARG;
    }
    for (uint32_t i = 0; i < n_keys; i++)
        if (keys[i] == SMX_STATS_EMPTY || flank_key_len(keys[i]) > SMX_FLANK_MAX_W) {
            snprintf(msg, sizeof msg, "key %u (%016llx) is no flank key", i, (unsigned long long)keys[i]);
            *why = msg;
            return SMX_ERR_ARG;
        }
    // the candidates grouped by primer, each group in the caller's order
    P.pstart.assign(FLANK_MAX_PRIMERS + 1, 0);
    P.clen.resize(n_cands);
    P.cidx.resize(n_cands);
    P.cmw.resize((size_t)n_cands * 4);
    for (uint32_t c = 0; c < n_cands; c++) {
        const uint32_t m = cand_off[c + 1] - cand_off[c];
        if (cand_off[c + 1] < cand_off[c] || m < 1 || m > SMX_FLANK_MAX_W) {
            snprintf(msg, sizeof msg, "candidate %u has %u letters (1..%d)", c, m, SMX_FLANK_MAX_W);
            *why = msg;
            return SMX_ERR_ARG;
        }
        if (cand_primer[c] >= FLANK_MAX_PRIMERS) {
            snprintf(msg, sizeof msg, "candidate %u names primer %u (0..%d)", c, cand_primer[c], FLANK_MAX_PRIMERS - 1);
            *why = msg;
            return SMX_ERR_ARG;
        }
        P.pstart[cand_primer[c] + 1]++;
    }
    for (int p = 0; p < FLANK_MAX_PRIMERS; p++) P.pstart[p + 1] += P.pstart[p];
    std::vector<int> at(P.pstart.begin(), P.pstart.end() - 1);
    for (uint32_t c = 0; c < n_cands; c++) {
        const int m = (int)(cand_off[c + 1] - cand_off[c]), s = at[cand_primer[c]]++;
        unsigned long long peq[16];
        std::string bad;
        if (!build_peq(cands + cand_off[c], m, peq, &bad)) {
            *why = "candidate " + std::to_string(c) + ": " + bad;
            return SMX_ERR_ARG;
        }
        for (int b = 0; b < 4; b++) P.cmw[(size_t)s * 4 + b] = (uint32_t)peq[b];   // codes 0..3 = A C G T
        P.clen[s] = m;
        P.cidx[s] = (int)c;
    }
    return SMX_OK;
}

}  // namespace smx

#endif  // SMX_FLANK_PLAN_H
