// The error-profile kernel of specimux_amd/csrc/smx_profile.hip as a host loop, for tests/cpu/profile_sim.cpp and
// tests/asan/profile_driver.cpp: the same grid, the same indices, the same batches of 64 columns with the same three
// carries and the same core functions (smx_profile_core.h), a wave being a loop over 64 lanes, its scans prefix loops
// and its shuffles array reads.  The buffers are the caller's, of exactly the sizes the plan (smx_cons_plan.h: cons_plan,
// cons_plan_profile) gives; `tables` must be zeroed, as the library zeroes the device's.
#ifndef PROFILE_HOST_H
#define PROFILE_HOST_H
#include <vector>

#include "smx_cons_plan.h"
#include "smx_profile_core.h"

namespace smx {

constexpr unsigned PROFILE_HOST_WAVES = 4;       // smx_profile.hip: PROFILE_WAVES

// bytes / off: the reads as the caller has them (the device has padded copies; the kernel reads the drafts' bytes only);
// quals in the same layout
inline void profile_host(const ConsPlan &P, const char *bytes, const uint64_t *off, const uint32_t *rows, const int32_t *dist,
                         const unsigned char *quals, uint32_t *per_member, uint32_t *tables) {
    const uint32_t n_jobs = (uint32_t)P.jobs.size();
    const uint32_t grid_y = (P.profile_max_members + SMX_PROFILE_BLOCK_MEMBERS - 1) / SMX_PROFILE_BLOCK_MEMBERS;
    for (uint32_t j = 0; j < n_jobs; j++)
        for (uint32_t by = 0; by < grid_y; by++) {
            const ConsJobDev &J = P.jobs[j];
            const uint32_t first = by * SMX_PROFILE_BLOCK_MEMBERS;
            if (first >= J.n) continue;
            uint32_t tab[SMX_PROFILE_JOB_WORDS] = {0};
            const uint32_t m = (uint32_t)P.len[J.draft];
            const unsigned char *draft = (const unsigned char *)bytes + off[J.draft];
            const auto add_tab = [&](unsigned at, uint32_t v) { tab[at] += v; };
            for (uint32_t wave = 0; wave < PROFILE_HOST_WAVES; wave++) {
                uint32_t wq[PROFILE_Q_WORDS] = {0};
                const auto add_wq = [&](unsigned at, uint32_t v) { wq[at - PROFILE_Q] += v; };
                for (uint32_t i = first + wave; i < J.n && i < first + SMX_PROFILE_BLOCK_MEMBERS; i += PROFILE_HOST_WAVES) {
                    uint32_t *out = per_member + (J.dist_off + i) * (uint64_t)SMX_PROFILE_MEMBER_WORDS;
                    if (dist[J.dist_off + i] < 0) {
                        for (unsigned x = 0; x < SMX_PROFILE_MEMBER_WORDS; x++) out[x] = 0u;
                        continue;
                    }
                    const uint32_t r = J.r0 + i;
                    const uint32_t *row = rows + J.rows_off + (uint64_t)i * ((uint64_t)m + 1u);
                    const unsigned char *qual = quals + off[r];
                    const uint32_t rlen = (uint32_t)(off[r + 1] - off[r]);
                    uint32_t n_match = 0, n_sub = 0, n_del = 0, n_other = 0, n_events = 0, clipped = 0;
                    uint32_t consumed = 0, open_start1 = 0, open_sum = 0;
                    for (uint32_t b0 = 0; b0 <= m; b0 += 64) {
                        uint32_t w[64], cls[64], L[64], c[64], share[64], incl[64], start1[64], sum[64];
                        unsigned dc[64];
                        bool ends[64];
                        for (unsigned lane = 0; lane < 64; lane++) {   // the loads and the ballots
                            const uint32_t p = b0 + lane;
                            w[lane] = p <= m ? row[p] : 0u;
                            const uint32_t wn = p < m ? row[p + 1] : 0u;
                            dc[lane] = p < m ? cons_code(draft[p]) : PROFILE_NO_CODE;
                            const unsigned dprev = p > 0 && p <= m ? cons_code(draft[p - 1]) : PROFILE_NO_CODE;
                            const unsigned dnext = p + 1 < m ? cons_code(draft[p + 1]) : PROFILE_NO_CODE;
                            cls[lane] = profile_class(w[lane], dc[lane], p, m);
                            L[lane] = p <= m ? profile_len(w[lane]) : 0u;
                            n_match += cls[lane] == PROFILE_MATCH;
                            n_sub += cls[lane] == PROFILE_SUB;
                            n_del += cls[lane] == PROFILE_DEL;
                            n_other += cls[lane] == PROFILE_OTHER;
                            n_events += L[lane] != 0u;
                            clipped |= L[lane] == 255u ? 1u : 0u;
                            const int at = profile_subst_index(w[lane], dc[lane], p, m);   // the kernel's diagonal included
                            if (at >= 0) add_tab((unsigned)at, 1u);
                            if (L[lane] != 0u) profile_ins(w[lane], add_tab);
                            ends[lane] = profile_ends_run(dc[lane], dnext, p, m);
                            c[lane] = profile_consumed(w[lane], p, m);
                            share[lane] = profile_run_votes(w[lane], wn, dc[lane], ends[lane], p, m);
                            const uint32_t packed = c[lane] | (share[lane] << 16);
                            incl[lane] = (lane ? incl[lane - 1] : 0u) + packed;
                            const uint32_t mine = profile_starts(dprev, dc[lane], p, m) ? p + 1u : 0u;
                            const uint32_t scan1 = lane && start1[lane - 1] > mine ? start1[lane - 1] : mine;
                            start1[lane] = scan1;                    // the carry joins below: max is associative
                        }
                        for (unsigned lane = 0; lane < 64; lane++) {   // after the scans
                            const uint32_t p = b0 + lane;
                            const uint32_t c_incl = incl[lane] & 0xffffu, s_incl = incl[lane] >> 16;
                            const uint32_t rp = consumed + (c_incl - c[lane]) + L[lane];
                            if (!clipped) profile_q(w[lane], cls[lane], rp, qual, rlen, add_wq);
                            if (start1[lane] < open_start1) start1[lane] = open_start1;
                            const uint32_t start = start1[lane] - 1u;
                            const unsigned from = start1[lane] != 0u && start >= b0 ? start - b0 : 0u;
                            const uint32_t excl_at_start = (incl[from] >> 16) - share[from];
                            sum[lane] = profile_stretch_sum(s_incl, excl_at_start, open_sum, start, b0);
                            if (ends[lane]) add_tab(profile_hp_index(p + 1u - start, sum[lane]), 1u);
                        }
                        consumed += incl[63] & 0xffffu;
                        open_start1 = start1[63];
                        open_sum = sum[63];
                    }
                    out[0] = n_match, out[1] = n_sub, out[2] = n_del, out[3] = n_other;
                    out[4] = n_events, out[5] = consumed - (n_match + n_sub + n_other), out[6] = clipped, out[7] = 0u;
                    for (unsigned x = 0; x < PROFILE_Q_WORDS; x++) {
                        if (!clipped) tab[PROFILE_Q + x] += wq[x];
                        wq[x] = 0u;
                    }
                }
            }
            for (unsigned x = 0; x < SMX_PROFILE_JOB_WORDS; x++) tables[(uint64_t)j * SMX_PROFILE_JOB_WORDS + x] += tab[x];
        }
}

}  // namespace smx

#endif  // PROFILE_HOST_H
