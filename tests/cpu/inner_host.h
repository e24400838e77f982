// The inner-scan kernels (specimux_amd/csrc/smx_inner.hip) as host loops over a planned call, shared by the CPU simulation
// (tests/cpu/inner_plan_sim.cpp) and the sanitizer driver (tests/asan/inner_driver.cpp).  It walks the plan
// (smx_inner_plan.h) the way inner_call does -- launch group after launch group, per group the scan of each word-width
// class over (unit, pass) and one merge over (read, pattern) -- and calls inner_scan_piece<W, G> and inner_merge
// exactly as the kernels do, with the kernels' own index expressions.  Every buffer is a heap allocation of its own of
// exactly the planned size; the bases end at the 16-byte word that holds the group's last byte, which is what
// inner_scan_piece says it reads, not the slack an upload may add.
#ifndef SMX_TESTS_INNER_HOST_H
#define SMX_TESTS_INNER_HOST_H
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "smx_inner_plan.h"

namespace smx {

[[noreturn]] inline void inner_host_fail(const char *what) {
    fprintf(stderr, "host twin: %s\n", what);
    exit(3);
}

// The IUPAC alphabet of the library's host code (smx_api.cpp is compiled with the device runtime; this is its table
// written out again): the 28 symmetric, non-transitive equalities plus identity.
inline bool inner_host_iupac_eq(unsigned char a, unsigned char b) {
    if (a == b) return true;
    static const char *pairs[] = {"YC", "YT", "RA", "RG", "NA", "NC", "NG", "NT", "WA", "WT", "MA", "MC", "SC", "SG",
                                  "KG", "KT", "BC", "BG", "BT", "DA", "DG", "DT", "HA", "HC", "HT", "VA", "VC", "VG"};
    for (const char *p : pairs)
        if (((unsigned char)p[0] == a && (unsigned char)p[1] == b) || ((unsigned char)p[0] == b && (unsigned char)p[1] == a)) return true;
    return false;
}

inline int inner_host_code_of(unsigned char ch) {
    for (int c = 0; c < 15; c++)
        if ((unsigned char)kCodeChars[c] == ch) return c;
    return 15;
}

inline bool inner_host_build_peq(const char *pat, int m, unsigned long long *peq16, std::string *bad) {
    for (int c = 0; c < 16; c++) peq16[c] = 0;
    for (int i = 0; i < m; i++) {
        const unsigned char pc = (unsigned char)pat[i];
        if (pc >= 128 || inner_host_code_of(pc) == 15) {
            if (bad) *bad = std::string("pattern character '") + (char)pc + "' is outside the IUPAC DNA alphabet";
            return false;
        }
        for (int c = 0; c < 15; c++)
            if (inner_host_iupac_eq(pc, (unsigned char)kCodeChars[c])) peq16[c] |= 1ull << i;
    }
    return true;
}

inline InnerAlphabet inner_host_alphabet() { return InnerAlphabet{inner_host_code_of, inner_host_build_peq}; }

struct InnerHostCounts {
    long long groups = 0, units = 0, scans = 0, merges = 0, reads = 0, groups_of_one = 0, groups_over_budget = 0;
    long long scans_g4 = 0, scans_g8 = 0, scans_w32 = 0, scans_w64 = 0, padding_slots = 0, passes_max = 0;
    long long last_word_loads = 0;      // units that read the last 16-byte word of their group's bases
};

// inner_scan_kernel<W, G> over the group's units and the class's passes
template <typename W, int G>
inline void inner_host_scan(const InnerPlan &P, const InnerClass &C, const InnerGroup &g, const std::vector<unsigned char> &lut,
                            const std::vector<mine_u4> &bases, const std::vector<uint64_t> &roff_v, const std::vector<uint32_t> &ustart,
                            const std::vector<uint32_t> &unit_read, std::vector<uint32_t> &recs, InnerHostCounts *counts) {
    const size_t slots = C.slots();
    // the class's tables as allocations of their own: what A.peq / A.pm / A.pk / A.jmap point at, to their ends
    std::vector<W> peq(slots * 16);
    memcpy(peq.data(), P.blob.data() + C.peq_at, peq.size() * sizeof(W));
    std::vector<int> pm(slots), pk(slots), jmap(slots);
    const int *tab = reinterpret_cast<const int *>(P.blob.data() + C.tab_at);
    for (size_t s = 0; s < slots; s++) { pm[s] = tab[s]; pk[s] = tab[slots + s]; jmap[s] = tab[2 * slots + s]; }
    const uint32_t n_units = (uint32_t)g.units;
    const uint64_t grid = ((uint64_t)n_units + INNER_THREADS - 1) / INNER_THREADS;
    for (size_t pass = 0; pass < (size_t)C.npass; pass++)            // blockIdx.y
        for (uint64_t block = 0; block < grid; block++) {             // blockIdx.x
            W s_peq[16 * G];
            unsigned char s_lut[256];
            int s_m[G], s_k[G], s_j[G];
            for (int tid = 0; tid < INNER_THREADS; tid++) {
                s_lut[tid] = lut[tid];
                if (tid < 16 * G) s_peq[tid] = peq[pass * 16 * G + tid];
                if (tid < G) {
                    s_m[tid] = pm[pass * G + tid];
                    s_k[tid] = pk[pass * G + tid];
                    s_j[tid] = jmap[pass * G + tid];
                }
            }
            for (int tid = 0; tid < INNER_THREADS; tid++) {
                const uint64_t unit = block * INNER_THREADS + tid;
                if (unit >= n_units) continue;
                const uint32_t r = unit_read[unit];
                const int piece = (int)((uint32_t)unit - ustart[r]);
                const uint64_t roff = roff_v[r];
                const int n = (int)(roff_v[r + 1] - roff);
                inner_scan_piece<W, G>(s_peq, s_lut, s_m, s_k, s_j, bases.data(), roff, n, P.margin, P.PL, P.lead, piece, (int)P.H,
                                       recs.data() + unit * (uint64_t)P.Q * (uint64_t)inner_rec_words((int)P.H));
                if (counts) {
                    counts->scans++;
                    const int end = std::min(n - P.margin, P.margin + (piece + 1) * P.PL);
                    if (end > 0 && ((roff + (uint64_t)end - 1) >> 4) + 1 == bases.size()) counts->last_word_loads++;
                }
            }
        }
    if (counts) {
        (G == 4 ? counts->scans_g4 : counts->scans_g8) += C.npass;
        (sizeof(W) == 4 ? counts->scans_w32 : counts->scans_w64) += C.npass;
        counts->padding_slots += (long long)(slots - C.idx.size());
        counts->passes_max = std::max<long long>(counts->passes_max, C.npass);
    }
}

// One call over reads seq[i][0 .. len[i]); flat: they lie back to back from seq[0], and a group is uploaded from there.
// nhit / hit_dist / hit_end: n_reads x Q (x H) entries, as the caller of the library hands them in.
inline void inner_host_run(const InnerPlan &P, const char *const *seq, const uint32_t *len, bool flat, uint32_t n_reads,
                           std::vector<uint8_t> *nhit, std::vector<int8_t> *hit_dist, std::vector<int32_t> *hit_end, InnerHostCounts *counts) {
    const uint32_t Q = P.Q, H = P.H;
    if (nhit->size() != (size_t)n_reads * Q || hit_dist->size() != (size_t)n_reads * Q * H || hit_end->size() != (size_t)n_reads * Q * H)
        inner_host_fail("the outputs are not n_reads x Q (x H)");
    const std::vector<unsigned char> lut(P.blob.begin(), P.blob.begin() + 256);
    InnerGroup g;
    std::string why;
    for (uint32_t r0 = 0; r0 < n_reads; r0 = g.r1) {
        if (P.next_group(len, n_reads, r0, &g, &why) != SMX_OK) inner_host_fail(why.c_str());
        if (g.r1 <= r0) inner_host_fail("a launch group without reads");
        const uint32_t nr = g.nr();
        // the uploads and the device buffers of the group, each of exactly the planned bytes
        if (g.bases_bytes % 16 || g.bases_bytes < g.nb) inner_host_fail("the bases do not end on a 16-byte word behind the last byte");
        std::vector<mine_u4> bases(g.bases_bytes / 16, mine_u4{0x2a2a2a2au, 0x2a2a2a2au, 0x2a2a2a2au, 0x2a2a2a2au});
        unsigned char *b = reinterpret_cast<unsigned char *>(bases.data());
        if (flat) {
            if (g.nb) memcpy(b, seq[r0], g.nb);
        } else {
            for (uint32_t i = 0; i < nr; i++)
                if (len[r0 + i]) memcpy(b + g.roff[i], seq[r0 + i], len[r0 + i]);
        }
        const std::vector<uint64_t> roff(g.roff);
        const std::vector<uint32_t> ustart(g.ustart), unit_read(g.unit_read);
        if (g.rec_bytes % 4) inner_host_fail("the records are not whole words");
        std::vector<uint32_t> recs(g.rec_bytes / 4, 0xdeadbeefu);       // the kernel's records start as junk too
        std::vector<unsigned char> out(g.out_bytes(), 0x55);
        if (g.he_bytes % 4) inner_host_fail("the hit ends are not whole words");
        // the carve of the output buffer: he | hd | nh (the heap aligns the buffer for the int32 part at its start)
        int32_t *d_he = reinterpret_cast<int32_t *>(out.data());
        int8_t *d_hd = reinterpret_cast<int8_t *>(out.data()) + g.he_bytes;
        uint8_t *d_nh = out.data() + g.he_bytes + g.hd_bytes;
        for (const InnerClass &C : P.cls) {
            if (C.idx.empty() || g.units == 0) continue;
            if (C.npass < 1 || C.npass > 65535) inner_host_fail("a pass count the launch refuses");
            if (C.G == 4) {
                if (C.w64) inner_host_scan<uint64_t, 4>(P, C, g, lut, bases, roff, ustart, unit_read, recs, counts);
                else inner_host_scan<uint32_t, 4>(P, C, g, lut, bases, roff, ustart, unit_read, recs, counts);
            } else if (C.G == 8) {
                if (C.w64) inner_host_scan<uint64_t, 8>(P, C, g, lut, bases, roff, ustart, unit_read, recs, counts);
                else inner_host_scan<uint32_t, 8>(P, C, g, lut, bases, roff, ustart, unit_read, recs, counts);
            } else {
                inner_host_fail("a G the launch refuses");
            }
        }
        // inner_merge_kernel
        for (uint64_t t = 0; t < (uint64_t)nr * (uint64_t)Q; t++) {
            const uint32_t r = (uint32_t)(t / (uint64_t)Q);
            const int j = (int)(t - (uint64_t)r * (uint64_t)Q);
            const uint32_t u0 = ustart[r];
            inner_merge(recs.data(), u0, (int)(ustart[r + 1] - u0), (int)Q, j, (int)H, P.margin, P.PL, d_nh + t, d_hd + t * H, d_he + t * H);
            if (counts) counts->merges++;
        }
        memcpy(hit_end->data() + (size_t)r0 * Q * H, d_he, g.he_bytes);
        memcpy(hit_dist->data() + (size_t)r0 * Q * H, d_hd, g.hd_bytes);
        memcpy(nhit->data() + (size_t)r0 * Q, d_nh, g.nh_bytes);
        if (counts) {
            counts->groups++;
            counts->units += (long long)g.units;
            counts->reads += nr;
            counts->groups_of_one += nr == 1;
            uint64_t longest = 0;
            for (uint32_t i = 0; i < nr; i++) longest = std::max<uint64_t>(longest, len[r0 + i]);
            counts->groups_over_budget += longest > P.budget;
        }
    }
}

}  // namespace smx

#endif  // SMX_TESTS_INNER_HOST_H
