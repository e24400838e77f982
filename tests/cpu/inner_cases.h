// The inner-scan shapes of the plan tests, shared by the CPU simulation (tests/cpu/inner_plan_sim.cpp, which checks every
// output against the definition of a hit over the whole read's last DP row) and the sanitizer driver
// (tests/asan/inner_driver.cpp): panels of 1 to 128 patterns in one and two word widths, reads from empty to 20 000
// bases around the piece boundaries, three budgets and both entries.
#ifndef SMX_TESTS_INNER_CASES_H
#define SMX_TESTS_INNER_CASES_H
#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "inner_host.h"

namespace smx {

struct InnerPanelCase {
    std::string pats;
    std::vector<uint32_t> poff{0};
    std::vector<int32_t> k;
    uint32_t Q() const { return (uint32_t)k.size(); }
    std::string pattern(uint32_t j) const { return pats.substr(poff[j], poff[j + 1] - poff[j]); }
    void add(const std::string &p, int kk) { pats += p; poff.push_back((uint32_t)pats.size()); k.push_back(kk); }
};

static const uint32_t kInnerQ[6] = {1, 4, 5, 8, 9, 128};

// Q = 1: one 40-nt pattern.  4: three of <= 32 nt and one longer (G = 4 twice).  5: five longer ones (G = 8, three
// padding slots).  8: four and four.  9: eight longer ones and a short one.  128: all <= 32 nt, 16 passes of 8.
inline InnerPanelCase inner_panel_case(uint32_t Q, std::mt19937 &rng) {
    static const int shorts[6] = {1, 12, 19, 22, 31, 32}, longs[4] = {33, 48, 63, 64};
    InnerPanelCase C;
    for (uint32_t j = 0; j < Q; j++) {
        bool is_long;
        switch (Q) {
            case 1: is_long = true; break;
            case 4: is_long = j == 2; break;
            case 5: is_long = true; break;
            case 8: is_long = j % 2 == 1; break;
            case 9: is_long = j != 4; break;
            default: is_long = false; break;
        }
        const int m = Q == 1 ? 40 : is_long ? longs[(j + rng()) % 4] : shorts[(j + rng()) % 6];
        std::string p(m, 'A');
        for (char &c : p) c = rng() % 9 == 0 ? "NRYKMSWBDHV"[rng() % 11] : "ACGT"[rng() % 4];
        const int kind = (int)(rng() % 3);
        C.add(p, std::min(m - 1, kind == 0 ? 0 : kind == 1 ? m / 6 : m / 4));
    }
    return C;
}

// a concrete read-side copy of a pattern with a few edits
inline std::string inner_copy(const std::string &p, int edits, std::mt19937 &rng) {
    std::string s = p;
    for (char &c : s) {
        char pick[4];
        int np = 0;
        for (char b : {'A', 'C', 'G', 'T'})
            if (inner_host_iupac_eq((unsigned char)c, (unsigned char)b)) pick[np++] = b;
        c = pick[rng() % np];
    }
    for (int e = 0; e < edits && !s.empty(); e++) {
        const size_t at = rng() % s.size();
        const int kind = (int)(rng() % 3);
        if (kind == 0) s[at] = "ACGT"[rng() % 4];
        else if (kind == 1) s.insert(s.begin() + at, "ACGT"[rng() % 4]);
        else if (s.size() > 1) s.erase(s.begin() + at);
    }
    return s;
}

// reads of 0, 1, 2 margin, 2 margin + 1, 2 margin + PL, 2 margin + PL + 1 and 20 000 bases, and three of a few hundred
inline std::vector<std::string> inner_reads_case(const InnerPanelCase &C, int margin, int PL, std::mt19937 &rng) {
    const int lens[10] = {0, 700, 1, 2 * margin, 20000, 2 * margin + 1, 2 * margin + PL, 333, 2 * margin + PL + 1, 1501};
    std::vector<std::string> reads;
    for (int n : lens) {
        std::string r(n, 'A');
        for (char &c : r) c = "ACGT"[rng() % 4];
        for (int at = 5; at + 170 < n; at += 90 + (int)(rng() % 120)) {      // copies, now and then two back to back
            const uint32_t j = rng() % C.Q();
            std::string ins = inner_copy(C.pattern(j), (int)(rng() % (C.k[j] + 2)), rng);
            if (rng() % 4 == 0) ins += inner_copy(C.pattern(j), 0, rng);
            r.replace(at, ins.size(), ins);
        }
        for (int i = 0; i < n / 100; i++) r[rng() % n] = "NRacgn\xff"[rng() % 7];   // bytes the code map has to get right
        r.resize(n);
        reads.push_back(r);
    }
    return reads;
}

// D(c) for every column c: the last row of the HW DP (row 0 is 0 everywhere), by the O(nm) recurrence
inline std::vector<int> inner_ref_last_row(const std::string &p, const std::string &t) {
    const int m = (int)p.size(), n = (int)t.size();
    std::vector<int> col(m + 1), out(n);
    for (int i = 0; i <= m; i++) col[i] = i;
    for (int j = 0; j < n; j++) {
        int diag = 0;
        const bool known = inner_host_code_of((unsigned char)t[j]) != 15;      // a byte outside the 15 letters matches nothing
        for (int i = 1; i <= m; i++) {
            const bool eq = known && inner_host_iupac_eq((unsigned char)p[i - 1], (unsigned char)t[j]);
            const int up = col[i - 1] + 1, left = col[i] + 1, sub = diag + (eq ? 0 : 1);
            diag = col[i];
            col[i] = std::min(std::min(up, left), sub);
        }
        out[j] = col[m];
    }
    return out;
}

// the definition, over the whole read: maximal runs of columns with D <= k inside [margin, n - margin), each reported
// at the first column of its least value
inline void inner_ref_hits(const std::vector<int> &D, int k, int margin, int H, uint8_t *nhit, int8_t *hd, int32_t *he, long long *runs) {
    const int n = (int)D.size();
    int total = 0;
    for (int h = 0; h < H; h++) { hd[h] = -1; he[h] = 0; }
    for (int c = margin; c < n - margin;) {
        if (D[c] > k) { c++; continue; }
        int best = D[c], end = c;
        for (c++; c < n - margin && D[c] <= k; c++)
            if (D[c] < best) { best = D[c]; end = c; }
        if (total < H) { hd[total] = (int8_t)best; he[total] = end; }
        total++;
    }
    *runs += total;
    *nhit = (uint8_t)std::min(total, 255);
}

struct InnerCaseTotals {
    InnerHostCounts H;
    long long calls = 0, compared = 0, mismatches = 0, runs = 0, more_than_H = 0, groupings = 0;
    long long groups_default = 0, groups_one_read = 0, groups_small = 0;
};

struct InnerOut {
    std::vector<uint8_t> nhit;
    std::vector<int8_t> hd;
    std::vector<int32_t> he;
    InnerOut(size_t n_reads, uint32_t Q, uint32_t H) : nhit(n_reads * Q, 0x77), hd(n_reads * Q * H, 0x77), he(n_reads * Q * H, 0x77777777) {}
    bool operator==(const InnerOut &o) const { return nhit == o.nhit && hd == o.hd && he == o.he; }
};

// Every panel x margin x H x budget x entry.  reference: compare with the definition; otherwise only across budgets and
// entries (the sanitizer driver).
inline void inner_cases_run(bool reference, InnerCaseTotals *totals) {
    InnerCaseTotals &Tt = *totals;
    std::mt19937 rng(99);
    for (uint32_t Q : kInnerQ) {
        const InnerPanelCase C = inner_panel_case(Q, rng);
        for (int margin : {0, 80}) {
            InnerPlan P0;
            std::string why;
            if (inner_plan(C.pats.data(), C.poff.data(), Q, C.k.data(), margin, 1, 0, INNER_DEFAULT_BUDGET, inner_host_alphabet(), &P0, &why) != SMX_OK)
                inner_host_fail(why.c_str());
            const std::vector<std::string> reads = inner_reads_case(C, margin, P0.PL, rng);
            const uint32_t n_reads = (uint32_t)reads.size();
            std::string flat;
            std::vector<uint32_t> len;
            for (const std::string &r : reads) { flat += r; len.push_back((uint32_t)r.size()); }
            std::vector<const char *> seq_flat, seq_own;
            size_t at = 0;
            for (const std::string &r : reads) { seq_flat.push_back(flat.data() + at); seq_own.push_back(r.data()); at += r.size(); }
            std::vector<std::vector<std::vector<int>>> D;      // [read][pattern]
            if (reference)
                for (const std::string &r : reads) {
                    D.emplace_back();
                    for (uint32_t j = 0; j < Q; j++) D.back().push_back(inner_ref_last_row(C.pattern(j), r));
                }
            for (uint32_t H : {1u, 8u}) {
                InnerOut want(n_reads, Q, H);
                if (reference)
                    for (uint32_t r = 0; r < n_reads; r++)
                        for (uint32_t j = 0; j < Q; j++) {
                            const size_t t = (size_t)r * Q + j;
                            long long runs = 0;
                            inner_ref_hits(D[r][j], C.k[j], margin, (int)H, &want.nhit[t], &want.hd[t * H], &want.he[t * H], &runs);
                            Tt.runs += runs;
                            Tt.more_than_H += runs > (long long)H;
                        }
                // the default, one read per group (any one read goes, whatever the budget), and less than the longest read
                const uint64_t budgets[3] = {0, 1, 10000};
                InnerOut first(n_reads, Q, H);
                for (int b = 0; b < 3; b++)
                    for (int entry = 0; entry < 2; entry++) {
                        InnerPlan P;
                        if (inner_plan(C.pats.data(), C.poff.data(), Q, C.k.data(), margin, H, budgets[b], INNER_DEFAULT_BUDGET,
                                       inner_host_alphabet(), &P, &why) != SMX_OK)
                            inner_host_fail(why.c_str());
                        InnerOut got(n_reads, Q, H);
                        InnerHostCounts HC;
                        inner_host_run(P, entry ? seq_own.data() : seq_flat.data(), len.data(), entry == 0, n_reads, &got.nhit, &got.hd, &got.he, &HC);
                        Tt.calls++;
                        if (b == 0 && entry == 0) first = got;
                        Tt.compared++;
                        if (!(got == first) && Tt.mismatches++ < 10)
                            fprintf(stderr, "MISMATCH Q=%u margin=%d H=%u budget %d entry %d: not the default budget's result\n", Q, margin, H, b, entry);
                        if (reference) {
                            for (size_t t = 0; t < (size_t)n_reads * Q; t++) {
                                Tt.compared++;
                                if ((want.nhit[t] != got.nhit[t] || memcmp(&want.hd[t * H], &got.hd[t * H], H) || memcmp(&want.he[t * H], &got.he[t * H], 4 * H)) &&
                                    Tt.mismatches++ < 10)
                                    fprintf(stderr, "MISMATCH Q=%u margin=%d H=%u budget %d entry %d read %zu (n=%u) pattern %zu: want n=%d d0=%d e0=%d, got n=%d d0=%d e0=%d\n",
                                            Q, margin, H, b, entry, t / Q, len[t / Q], t % Q, want.nhit[t], want.hd[t * H], want.he[t * H], got.nhit[t], got.hd[t * H], got.he[t * H]);
                            }
                        }
                        if (HC.reads != n_reads) inner_host_fail("the groups do not cover the reads once");
                        (b == 0 ? Tt.groups_default : b == 1 ? Tt.groups_one_read : Tt.groups_small) += HC.groups;
                        if (b == 1 && HC.groups != n_reads) inner_host_fail("a budget of one byte did not put one read in each group");
                        if (b == 0 && HC.groups != 1) inner_host_fail("the default budget split ten reads");
                        Tt.H.groups += HC.groups; Tt.H.units += HC.units; Tt.H.scans += HC.scans; Tt.H.merges += HC.merges;
                        Tt.H.groups_of_one += HC.groups_of_one; Tt.H.groups_over_budget += HC.groups_over_budget;
                        Tt.H.scans_g4 += HC.scans_g4; Tt.H.scans_g8 += HC.scans_g8; Tt.H.scans_w32 += HC.scans_w32; Tt.H.scans_w64 += HC.scans_w64;
                        Tt.H.padding_slots += HC.padding_slots; Tt.H.passes_max = std::max(Tt.H.passes_max, HC.passes_max);
                        Tt.H.last_word_loads += HC.last_word_loads;
                    }
            }
        }
    }
}

inline void inner_cases_print(const InnerCaseTotals &T) {
    printf("calls %lld\ngroups %lld\ngroups_default %lld\ngroups_one_read %lld\ngroups_small %lld\ngroups_of_one %lld\ngroups_over_budget %lld\n"
           "units %lld\nscans %lld\nmerges %lld\nscans_g4 %lld\nscans_g8 %lld\nscans_w32 %lld\nscans_w64 %lld\npadding_slots %lld\npasses_max %lld\n"
           "last_word_loads %lld\ncompared %lld\nruns %lld\nmore_than_H %lld\n",
           T.calls, T.H.groups, T.groups_default, T.groups_one_read, T.groups_small, T.H.groups_of_one, T.H.groups_over_budget, T.H.units,
           T.H.scans, T.H.merges, T.H.scans_g4, T.H.scans_g8, T.H.scans_w32, T.H.scans_w64, T.H.padding_slots, T.H.passes_max,
           T.H.last_word_loads, T.compared, T.runs, T.more_than_H);
    printf("%lld mismatches\n", T.mismatches);
}

}  // namespace smx

#endif  // SMX_TESTS_INNER_CASES_H
