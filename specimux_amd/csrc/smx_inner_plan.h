// smx_inner_plan.h -- the host-side plan of one smx_inner_scan* call (smx_calls.cpp): the pattern checks, lead / PL / RW,
// the table blob (byte -> code map, then per word-width class the match words [pass][code][G] and pm / pk / jmap), and
// the launch groups of whole reads under the budget with their unit prefix and buffer sizes.  Host
// only and free of HIP calls, so that the CPU simulation (tests/cpu/inner_plan_sim.cpp) and the sanitizer driver
// (tests/asan/inner_driver.cpp) run it as it is.  The IUPAC alphabet lives in smx_api.cpp, which is not: the plan takes
// it as two functions.
#ifndef SMX_INNER_PLAN_H
#define SMX_INNER_PLAN_H
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "smx_blob.h"
#include "smx_internal.h"

namespace smx {

constexpr uint64_t INNER_DEFAULT_BUDGET = (uint64_t)1 << 30;    // device bytes of one launch group when the caller names none

struct InnerAlphabet {
    int (*code_of)(unsigned char ch);                                                           // 0..14, 15 = other
    bool (*build_peq)(const char *pat, int m, unsigned long long *peq16, std::string *bad);    // false: a letter outside the alphabet
};

struct InnerClass {      // the patterns of one word width, in passes of G
    int w64 = 0, G = 4, npass = 0;
    std::vector<uint32_t> idx;        // pattern indices of the call
    size_t peq_at = 0, tab_at = 0;    // offsets into the table blob: match words; pm, pk, jmap (npass * G ints each)
    size_t slots() const { return (size_t)npass * G; }
};

// One launch group: the reads [r0, r1) and everything its launches and copies need.
struct InnerGroup {
    uint32_t r0 = 0, r1 = 0;
    uint64_t units = 0;                    // (read, piece) units of the group
    std::vector<uint64_t> roff;            // nr + 1 byte offsets of the reads, back to back
    std::vector<uint32_t> ustart;          // nr + 1: first unit of each read
    std::vector<uint32_t> unit_read;       // per unit: its read within the group
    // bases_bytes: the reads' bytes up to the end of the 16-byte word that holds the last one (what inner_scan_piece
    // loads); rec_bytes: units x Q records; he | hd | nh: the carve of the output buffer
    size_t nb = 0, bases_bytes = 0, rec_bytes = 0, he_bytes = 0, hd_bytes = 0, nh_bytes = 0;
    uint32_t nr() const { return r1 - r0; }
    size_t out_bytes() const { return he_bytes + hd_bytes + nh_bytes; }
};

struct InnerPlan {
    uint32_t Q = 0, H = 0;
    int32_t margin = 0;
    int lead = 1, PL = 64, RW = 3;
    InnerClass cls[2];
    std::vector<unsigned char> blob;       // what goes to the device in one piece; the byte -> code map at 0
    uint64_t budget = INNER_DEFAULT_BUDGET;

    // pieces of a read of n bases: its internal columns [margin, n - margin) in pieces of PL
    uint64_t pieces_of(uint32_t n) const {
        return (uint64_t)n > 2 * (uint64_t)margin ? ((uint64_t)n - 2 * (uint64_t)margin + PL - 1) / PL : 0;
    }

    // The group that starts at read r0 < n_reads: whole reads while everything one launch group keeps on the device
    // fits the budget (one read always goes).  Returns SMX_OK, or the status to fail with and why.
    int next_group(const uint32_t *len, uint32_t n_reads, uint32_t r0, InnerGroup *group, std::string *why) const {
        InnerGroup &g = *group;
        const uint64_t out_per_read = (uint64_t)Q * (1 + 5 * (uint64_t)H);
        uint64_t bytes = 64, units = 0, nb = 0;
        uint32_t r1 = r0;
        while (r1 < n_reads) {
            if (len[r1] > (uint32_t)INT32_MAX) {
                *why = "read " + std::to_string(r1) + ": longer than 2^31 - 1 bases";
                return SMX_ERR_ARG;
            }
            const uint64_t np = pieces_of(len[r1]);
            const uint64_t cost = (uint64_t)len[r1] + 12 + np * (4 + (uint64_t)Q * RW * 4) + out_per_read;
            if (r1 > r0 && (bytes + cost > budget || units + np > 0x7fffffffull)) break;
            bytes += cost;
            units += np;
            nb += len[r1];
            r1++;
        }
        if (units > 0xffffffffull) {
            *why = "read " + std::to_string(r0) + ": too many pieces for one launch";
            return SMX_ERR_UNSUPPORTED;
        }
        g.r0 = r0;
        g.r1 = r1;
        g.units = units;
        const uint32_t nr = r1 - r0;
        g.roff.resize((size_t)nr + 1);
        g.ustart.resize((size_t)nr + 1);
        g.unit_read.resize((size_t)units);
        g.roff[0] = 0;
        g.ustart[0] = 0;
        for (uint32_t i = 0; i < nr; i++) {
            const uint32_t np = (uint32_t)pieces_of(len[r0 + i]);
            g.roff[i + 1] = g.roff[i] + len[r0 + i];
            for (uint32_t p = 0; p < np; p++) g.unit_read[(size_t)g.ustart[i] + p] = i;
            g.ustart[i + 1] = g.ustart[i] + np;
        }
        g.nb = (size_t)nb;
        g.bases_bytes = ((size_t)nb + 15) & ~(size_t)15;
        g.rec_bytes = (size_t)units * Q * RW * 4;
        g.he_bytes = (size_t)nr * Q * H * 4;
        g.hd_bytes = (size_t)nr * Q * H;
        g.nh_bytes = (size_t)nr * Q;
        return SMX_OK;
    }
};

// The plan of a call.  budget = 0: default_budget (INNER_DEFAULT_BUDGET in production).  Returns SMX_OK, or the status
// to fail with and why.
inline int inner_plan(const char *patterns, const uint32_t *poff, uint32_t Q, const int32_t *k, int32_t margin, uint32_t H,
                      uint64_t budget, uint64_t default_budget, const InnerAlphabet &alphabet, InnerPlan *plan, std::string *why) {
    InnerPlan &P = *plan;
    P = InnerPlan();
    if (Q < 1 || Q > INNER_MAX_PATTERNS) {
        *why = "n_patterns " + std::to_string(Q) + " outside 1.." + std::to_string(INNER_MAX_PATTERNS);
        return SMX_ERR_ARG;
    }
    if (H < 1 || H > INNER_MAX_HITS) {
        *why = "max_hits " + std::to_string(H) + " outside 1.." + std::to_string(INNER_MAX_HITS);
        return SMX_ERR_ARG;
    }
    if (margin < 0) {
        *why = "margin " + std::to_string(margin) + " is negative";
        return SMX_ERR_ARG;
    }
    std::vector<unsigned long long> peq((size_t)Q * 16);
    std::vector<int> pm(Q);
    P.cls[1].w64 = 1;
    for (uint32_t j = 0; j < Q; j++) {
        if (poff[j + 1] <= poff[j] || poff[j + 1] - poff[j] > 64) {
            *why = "pattern " + std::to_string(j) + ": length outside 1..64";
            return SMX_ERR_ARG;
        }
        const int m = (int)(poff[j + 1] - poff[j]);
        if (k[j] < 0 || k[j] >= m) {
            *why = "pattern " + std::to_string(j) + ": threshold " + std::to_string(k[j]) + " outside 0.." + std::to_string(m - 1);
            return SMX_ERR_ARG;
        }
        std::string bad;
        if (!alphabet.build_peq(patterns + poff[j], m, &peq[(size_t)j * 16], &bad)) {
            *why = "pattern " + std::to_string(j) + ": " + bad;
            return SMX_ERR_ARG;
        }
        pm[j] = m;
        P.lead = std::max(P.lead, m + k[j]);
        P.cls[m > 32 ? 1 : 0].idx.push_back(j);
    }
    P.Q = Q;
    P.H = H;
    P.margin = margin;
    P.PL = inner_piece_len(P.lead);
    P.RW = inner_rec_words((int)H);
    P.budget = budget ? budget : default_budget;
    // pattern tables: byte -> code map, then per class the match words [pass][code][G] and pm / pk / jmap
    P.blob.resize(256);
    for (int c = 0; c < 256; c++) P.blob[c] = (unsigned char)alphabet.code_of((unsigned char)c);
    for (InnerClass &C : P.cls) {
        if (C.idx.empty()) continue;
        C.G = C.idx.size() <= 4 ? 4 : 8;
        C.npass = (int)((C.idx.size() + C.G - 1) / C.G);
        const size_t slots = C.slots();
        std::vector<int> tab(3 * slots);
        for (size_t s = 0; s < slots; s++) {
            const bool real = s < C.idx.size();
            tab[s] = real ? pm[C.idx[s]] : 1;
            tab[slots + s] = real ? k[C.idx[s]] : -1;
            tab[2 * slots + s] = real ? (int)C.idx[s] : -1;
        }
        if (C.w64) {
            std::vector<uint64_t> w(slots * 16, 0);
            for (size_t s = 0; s < C.idx.size(); s++)
                for (int c = 0; c < 16; c++) w[((s / C.G) * 16 + c) * C.G + s % C.G] = peq[(size_t)C.idx[s] * 16 + c];
            C.peq_at = blob_add(P.blob, w);
        } else {
            std::vector<uint32_t> w(slots * 16, 0);
            for (size_t s = 0; s < C.idx.size(); s++)
                for (int c = 0; c < 16; c++) w[((s / C.G) * 16 + c) * C.G + s % C.G] = (uint32_t)peq[(size_t)C.idx[s] * 16 + c];
            C.peq_at = blob_add(P.blob, w);
        }
        C.tab_at = blob_add(P.blob, tab);
    }
    return SMX_OK;
}

}  // namespace smx

#endif  // SMX_INNER_PLAN_H
