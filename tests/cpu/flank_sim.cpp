// CPU simulation of the barcode survey's kernels (specimux_amd/csrc/smx_flank.hip): the same per-hit and per-key code
// (smx_flank_core.h: flank_of_hit, flank_shw, flank_take, and smx_stats_core.h's table) against plain string code -- an
// ordinary reverse complement and a slice for the flank, a full DP matrix for the distance.  No GPU needed.
//
//   flank_sim flank            geometry, the four ways out, keys, and the count kernel's shape (workgroup chunks of hits
//                              counted into a small local table that is flushed into the global one) against a std::map
//   flank_sim exhaustive       every {A,C} candidate of 1-5 letters x every {A,C,G} flank of 0-7 letters x every k
//   flank_sim random SEED      13-letter (and 1..26-letter) candidates, planted copies at distance exactly k and k + 1,
//                              IUPAC candidates; writes oracle_sample.txt (candidate hex, flank hex, distance)
//   flank_sim plan             the host plan of smx_flank_assign (smx_flank_plan.h: argument checks, candidates regrouped
//                              by primer) against a plain stable sort by primer, and every refusal (flank_plan_host.h)
// Prints "name value" counters and, last, "N mismatches".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "smx_flank_core.h"
#include "flank_plan_host.h"

using namespace smx;

static long mismatches = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (mismatches++ < 20) { printf("MISMATCH " __VA_ARGS__); printf("\n"); } } } while (0)

// ---- plain reference code
static int iupac_mask(char c) {   // bit 0 A, 1 C, 2 G, 3 T
    switch (c) {
        case 'A': return 1; case 'C': return 2; case 'G': return 4; case 'T': return 8;
        case 'R': return 5; case 'Y': return 10; case 'K': return 12; case 'M': return 3; case 'S': return 6; case 'W': return 9;
        case 'B': return 14; case 'D': return 13; case 'H': return 11; case 'V': return 7; case 'N': return 15;
    }
    return 0;
}
static int base_index(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

static void match_words(const std::string &cand, uint32_t mw[4]) {
    for (int b = 0; b < 4; b++) mw[b] = 0;
    for (size_t i = 0; i < cand.size(); i++)
        for (int b = 0; b < 4; b++)
            if (iupac_mask(cand[i]) >> b & 1) mw[b] |= 1u << i;
}

static int dp_shw(const std::string &c, const std::string &f) {   // min over prefixes f[:j], 0 <= j <= len(f), of NW(c, f[:j])
    const int m = (int)c.size(), n = (int)f.size();
    std::vector<std::vector<int>> D(m + 1, std::vector<int>(n + 1));
    for (int i = 0; i <= m; i++) D[i][0] = i;
    for (int j = 0; j <= n; j++) D[0][j] = j;
    for (int i = 1; i <= m; i++)
        for (int j = 1; j <= n; j++) {
            const int sub = D[i - 1][j - 1] + ((iupac_mask(c[i - 1]) >> base_index(f[j - 1]) & 1) ? 0 : 1);
            D[i][j] = std::min(sub, std::min(D[i - 1][j] + 1, D[i][j - 1] + 1));
        }
    int best = D[m][0];
    for (int j = 1; j <= n; j++) best = std::min(best, D[m][j]);
    return best;
}

static std::string revcomp(const std::string &s) {
    static const char *from = "ACGTNacgtn", *to = "TGCANtgcan";
    std::string out(s.rbegin(), s.rend());
    for (char &ch : out) {
        const char *at = strchr(from, ch);
        if (at && ch) ch = to[at - from];
    }
    return out;
}

static uint64_t bits_of(const std::string &f) {
    uint64_t b = 0;
    for (size_t t = 0; t < f.size(); t++) b |= (uint64_t)base_index(f[t]) << (2 * t);
    return b;
}

static std::string hex(const std::string &s) {
    static const char *d = "0123456789abcdef";
    std::string out;
    for (unsigned char ch : s) { out += d[ch >> 4]; out += d[ch & 15]; }
    return out.empty() ? "-" : out;
}

// ---- mode flank
static int run_flank() {
    std::mt19937_64 rng(20240607);
    long n_hits = 0, cat_n[SMX_FLANK_N_COUNTERS] = {0}, w26 = 0, counted_a = 0, counted_b = 0, overlap_reads = 0, spilled = 0,
         every_jend = 0, repeated = 0;
    for (int S : {80, 31})
        for (int Lb : {8, 13, 23}) {
            const FlankPanel P = {3, S, Lb, 3};
            const int W = Lb + 3, H = 2 * P.NP, stride = (2 * S + 15) & ~15;
            std::vector<smx_hit> hits;
            std::vector<int32_t> lens;
            std::vector<uint8_t> windows;
            std::map<uint64_t, uint64_t> want;
            std::vector<uint64_t> want_ctr((size_t)P.NP * SMX_FLANK_N_COUNTERS, 0);
            std::vector<char> seen((size_t)2 * S, 0);
            for (int L : {S, S + 1, 2 * S - 1, S - 1, 20}) {
                std::vector<std::string> pool(3);
                for (std::string &r : pool) { r.resize(L); for (char &ch : r) ch = "ACGT"[rng() & 3]; }
                for (int rep = 0; rep < 3; rep++)
                    for (int j0 = 0; j0 < S; j0++) {
                        std::string read = pool[(size_t)(rng() % pool.size())];
                        const int variant = (int)(rng() % 8);
                        if (variant == 1) read[(size_t)(rng() % L)] = 'N';
                        if (variant == 2) read[(size_t)(rng() % L)] = 'a';
                        overlap_reads += L >= S && L < 2 * S;
                        const int Sp = std::min(S, L);
                        std::vector<uint8_t> row(stride, 0);
                        memcpy(&row[0], read.data(), Sp);
                        memcpy(&row[S], read.data() + L - Sp, Sp);
                        windows.insert(windows.end(), row.begin(), row.end());
                        lens.push_back(L);
                        for (int p = 0; p < P.NP; p++)
                            for (int e = 0; e < 2; e++) {
                                const int j_end = (j0 + 7 * p + 3 * e) % S;
                                smx_hit h;
                                memset(&h, 0, sizeof h);
                                h.pdist = (rng() % 16 == 0) ? -1 : (int16_t)(rng() % 3);
                                h.bbest = (rng() % 16 == 0) ? -2 : (rng() & 1) ? -1 : (int16_t)(rng() % 4);
                                h.first_end = j_end + (L - S);
                                h.nloc = 1;
                                hits.push_back(h);
                                // the plain statement of the definition
                                if (h.pdist < 0) continue;
                                n_hits++;
                                int cat;
                                std::string fl;
                                if (h.bbest == -2) cat = SMX_FLANK_PRUNED;
                                else if (L < S) cat = SMX_FLANK_SHORT_READ;
                                else {
                                    const std::string es = e ? read : revcomp(read);
                                    fl = es.substr((size_t)h.first_end + 1, (size_t)W);
                                    bool acgt = true;
                                    for (char ch : fl) acgt = acgt && base_index(ch) >= 0;
                                    cat = (int)fl.size() < Lb - 3 ? SMX_FLANK_SHORT_FLANK : !acgt ? SMX_FLANK_AMBIGUOUS : SMX_FLANK_COUNTED;
                                    seen[(size_t)e * S + j_end] = 1;
                                }
                                want_ctr[(size_t)p * SMX_FLANK_N_COUNTERS + cat]++;
                                want_ctr[(size_t)p * SMX_FLANK_N_COUNTERS + SMX_FLANK_HITS]++;
                                cat_n[cat]++;
                                if (cat == SMX_FLANK_COUNTED) {
                                    const uint64_t key = bits_of(fl) | (uint64_t)fl.size() << 52 | (uint64_t)(h.bbest >= 0) << 57 | (uint64_t)p << 58;
                                    want[key]++;
                                    w26 += fl.size() == 26;
                                    (e ? counted_b : counted_a)++;
                                }
                            }
                    }
            }
            for (char s : seen) every_jend += s;
            // the count kernel's shape
            const int grid = 3;
            const uint32_t cap = 1u << 16;
            std::vector<uint64_t> gkeys(cap, SMX_STATS_EMPTY), gcounts(cap, 0), ctr((size_t)P.NP * SMX_FLANK_N_COUNTERS, 0);
            uint64_t dropped = 0;
            auto global_add = [&](uint64_t key, uint64_t add) {
                const int s = stats_find_slot(gkeys.data(), cap, key, cap < STATS_GPROBE_MAX ? cap : STATS_GPROBE_MAX);
                if (s >= 0) gcounts[s] += add; else dropped += add;
            };
            const long n_items = (long)lens.size() * H;
            for (int b = 0; b < grid; b++) {
                std::vector<uint64_t> lkeys(FLANK_LCAP, SMX_STATS_EMPTY);
                std::vector<unsigned> lcnt(FLANK_LCAP, 0), lctr((size_t)64 * SMX_FLANK_N_COUNTERS, 0);
                for (long base = (long)b * FLANK_THREADS; base < n_items; base += (long)grid * FLANK_THREADS)
                    for (long it = base; it < base + FLANK_THREADS && it < n_items; it++) {
                        const long i = it / H;
                        const int pe = (int)(it - i * H);
                        uint64_t key = 0;
                        const int cat = flank_of_hit(P, hits[it], pe >> 1, pe & 1, lens[i], &windows[(size_t)i * stride], &key);
                        if (cat == 0) continue;
                        lctr[(size_t)(pe >> 1) * SMX_FLANK_N_COUNTERS + cat]++;
                        if (cat != SMX_FLANK_COUNTED) continue;
                        const int s = stats_find_slot(lkeys.data(), FLANK_LCAP, key, FLANK_LPROBE);
                        if (s >= 0) lcnt[s]++; else { spilled++; global_add(key, 1); }
                    }
                for (int s = 0; s < FLANK_LCAP; s++)
                    if (lkeys[s] != SMX_STATS_EMPTY && lcnt[s]) global_add(lkeys[s], lcnt[s]);
                for (int p = 0; p < P.NP; p++) {
                    uint64_t sum = 0;
                    for (int c = 1; c < SMX_FLANK_N_COUNTERS; c++) { ctr[(size_t)p * SMX_FLANK_N_COUNTERS + c] += lctr[(size_t)p * SMX_FLANK_N_COUNTERS + c]; sum += lctr[(size_t)p * SMX_FLANK_N_COUNTERS + c]; }
                    ctr[(size_t)p * SMX_FLANK_N_COUNTERS] += sum;
                }
            }
            CHECK(dropped == 0, "dropped %llu", (unsigned long long)dropped);
            CHECK(ctr == want_ctr, "counters differ S=%d Lb=%d", S, Lb);
            std::map<uint64_t, uint64_t> got;
            for (uint32_t s = 0; s < cap; s++)
                if (gkeys[s] != SMX_STATS_EMPTY) got[gkeys[s]] = gcounts[s];
            CHECK(got == want, "tables differ S=%d Lb=%d: %zu keys, %zu expected", S, Lb, got.size(), want.size());
            for (const auto &kv : want) repeated += kv.second > 1;
        }
    printf("hits %ld\npruned %ld\nshort_read %ld\nshort_flank %ld\nambiguous %ld\ncounted %ld\n", n_hits, cat_n[SMX_FLANK_PRUNED],
           cat_n[SMX_FLANK_SHORT_READ], cat_n[SMX_FLANK_SHORT_FLANK], cat_n[SMX_FLANK_AMBIGUOUS], cat_n[SMX_FLANK_COUNTED]);
    printf("w26 %ld\ncounted_a %ld\ncounted_b %ld\noverlap_reads %ld\nlocal_spill %ld\nend_positions %ld\nrepeated_keys %ld\n", w26,
           counted_a, counted_b, overlap_reads, spilled, every_jend, repeated);
    return 0;
}

// ---- mode exhaustive
static void check_assign(const std::vector<std::string> &cands, const std::string &flank, int kmax, long *cases) {
    const uint64_t bits = bits_of(flank);
    std::vector<int> d(cands.size());
    for (size_t c = 0; c < cands.size(); c++) {
        uint32_t mw[4];
        match_words(cands[c], mw);
        d[c] = flank_shw(mw, (int)cands[c].size(), bits, (int)flank.size());
        const int want = dp_shw(cands[c], flank);
        CHECK(d[c] == want, "shw %s vs %s: %d, DP %d", cands[c].c_str(), flank.c_str(), d[c], want);
        (*cases)++;
    }
    for (int k = 0; k <= kmax; k++) {
        FlankBest r = {-1, -1, 0};
        for (size_t c = 0; c < cands.size(); c++) flank_take(r, d[c], k, (int)c);
        int best = -1, first = -1, ntied = 0;
        for (size_t c = 0; c < cands.size(); c++) if (d[c] <= k && (best < 0 || d[c] < best)) best = d[c];
        for (size_t c = 0; c < cands.size(); c++) if (best >= 0 && d[c] == best) { if (first < 0) first = (int)c; ntied++; }
        CHECK(r.best == best && r.first == first && r.ntied == ntied, "assign %s k=%d: %d %d %d, plain %d %d %d", flank.c_str(), k,
              r.best, r.first, r.ntied, best, first, ntied);
    }
}

static int run_exhaustive() {
    std::vector<std::string> cands, flanks;
    for (int m = 1; m <= 5; m++)
        for (int v = 0; v < (1 << m); v++) {
            std::string s(m, 'A');
            for (int i = 0; i < m; i++) if (v >> i & 1) s[i] = 'C';
            cands.push_back(s);
        }
    for (int n = 0; n <= 7; n++) {
        int total = 1;
        for (int i = 0; i < n; i++) total *= 3;
        for (int v = 0; v < total; v++) {
            std::string s(n, 'A');
            for (int i = 0, x = v; i < n; i++, x /= 3) s[i] = "ACG"[x % 3];
            flanks.push_back(s);
        }
    }
    long cases = 0;
    for (const std::string &f : flanks) check_assign(cands, f, 5, &cases);
    printf("candidates %zu\nflanks %zu\ncases %ld\nassignments %zu\n", cands.size(), flanks.size(), cases, flanks.size() * 6);
    return 0;
}

// ---- mode random
static int run_random(unsigned long seed) {
    std::mt19937_64 rng(seed);
    auto rnd = [&](int n) { return (int)(rng() % (unsigned long)n); };
    auto random_acgt = [&](int n) { std::string s(n, 'A'); for (char &ch : s) ch = "ACGT"[rnd(4)]; return s; };
    FILE *fh = fopen("oracle_sample.txt", "w");
    if (!fh) { perror("oracle_sample.txt"); return 2; }
    long cases = 0, at_k = 0, at_k1 = 0, exact = 0, iupac = 0, len26 = 0, flank26 = 0, sample = 0, within = 0, ties = 0;
    static const char *deg = "RYKMSWBDHVN";
    for (int round = 0; round < 400; round++) {
        const int k = rnd(5);
        const bool wide = round % 4 == 3;                 // one round in four: lengths 1..26 instead of 13
        const int m = wide ? 1 + rnd(26) : 13;
        std::vector<std::string> cands;
        for (int c = 0; c < 24; c++) {
            std::string s = random_acgt(m);
            if (round % 3 == 2) for (int x = 0; x < 1 + rnd(3); x++) s[(size_t)rnd(m)] = deg[rnd(11)];
            cands.push_back(s);
        }
        if (round % 5 == 0) { const std::string dup = cands[(size_t)rnd(24)]; cands.push_back(dup); }   // a duplicate: a sure tie
        for (int t = 0; t < 40; t++) {
            // a planted copy: an instance of one candidate with e random edits, then random bases behind it
            const std::string &src = cands[(size_t)rnd((int)cands.size())];
            std::string f;
            for (char ch : src) { const int mask = iupac_mask(ch); int b; do b = rnd(4); while (!(mask >> b & 1)); f += "ACGT"[b]; }
            const int edits = t % 4 == 0 ? 0 : rnd(k + 3);
            for (int x = 0; x < edits && !f.empty(); x++) {
                const int kind = rnd(3), at = rnd((int)f.size());
                if (kind == 0) f[(size_t)at] = "ACGT"[(base_index(f[(size_t)at]) + 1 + rnd(3)) & 3];
                else if (kind == 1) f.insert((size_t)at, 1, "ACGT"[rnd(4)]);
                else f.erase((size_t)at, 1);
            }
            f += random_acgt(rnd(6));
            if (t % 8 == 7) f = f.substr(0, (size_t)rnd((int)f.size() + 1));    // a truncated flank
            if (f.size() > 26) f.resize(26);
            const int d_src = dp_shw(src, f);
            at_k += d_src == k; at_k1 += d_src == k + 1; exact += d_src == 0; within += d_src <= k;
            for (char ch : src) if (base_index(ch) < 0) { iupac++; break; }
            len26 += m == 26; flank26 += f.size() == 26;
            const long before = mismatches;
            check_assign(cands, f, k, &cases);
            {   // ties under this k
                int best = 99, nt = 0;
                for (const std::string &c : cands) { const int d = dp_shw(c, f); if (d < best) { best = d; nt = 1; } else if (d == best) nt++; }
                ties += best <= k && nt > 1;
            }
            if (before == mismatches && (round * 40 + t) % 37 == 0) {
                fprintf(fh, "%s %s %d\n", hex(src).c_str(), hex(f).c_str(), d_src);
                sample++;
            }
        }
    }
    fclose(fh);
    printf("cases %ld\nkind_at_k %ld\nkind_at_k_plus_1 %ld\nkind_exact %ld\nkind_within_k %ld\niupac_candidates %ld\n", cases, at_k, at_k1,
           exact, within, iupac);
    printf("len_26 %ld\nflank_26 %ld\nties %ld\noracle_sample %ld\n", len26, flank26, ties, sample);
    return 0;
}

// ---- mode plan
static int run_plan() {
    FlankPlanCounts C;
    flank_plan_cases(&C);
    flank_plan_print(C);
    mismatches += C.mismatches;
    return 0;
}

int main(int argc, char **argv) {
    int rc = 2;
    if (argc >= 2 && !strcmp(argv[1], "flank")) rc = run_flank();
    else if (argc >= 2 && !strcmp(argv[1], "exhaustive")) rc = run_exhaustive();
    else if (argc >= 3 && !strcmp(argv[1], "random")) rc = run_random(strtoul(argv[2], nullptr, 10));
    else if (argc >= 2 && !strcmp(argv[1], "plan")) rc = run_plan();
    else fprintf(stderr, "usage: flank_sim flank | exhaustive | random SEED | plan\n");
    if (rc) return rc;
    printf("%ld mismatches\n", mismatches);
    return mismatches ? 1 : 0;
}
