// CPU simulation of the inner scan's per-lane code (specimux_amd/csrc/smx_inner_core.h): the same host/device
// inner_scan_piece and inner_merge the gfx950 kernels of smx_inner.hip run, over tables built the way smx_calls.cpp's
// inner_call builds them (byte -> code map, match words [pass][code][G], 32-bit words for patterns up to 32 letters and
// 64-bit words above), checked against a plain last-row DP and the definition of a hit applied to the whole read.
// Built and run by tests/test_inner_cpu.py (g++, no GPU).
//
//   inner_sim exhaustive        every {A, C} pattern of length 1-5 x every {A, C, N} read of length 0-9 x margin 0-3 x
//                               every valid k x H in {1, 3}, at the kernel's piece length and, for every fourth read,
//                               in pieces of 1-3 columns; calls of up to 43 (pattern, k) slots, a few threads
//   inner_sim random <seed>     structured random cases (see run_random), writes oracle_sample.txt in the cwd
//
// Prints "<counter> <value>" lines (the Python test asserts lower bounds on them) and "<n> mismatches".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "smx_inner_core.h"

using namespace smx;
typedef std::string Seq;

static const char kCodes[16] = {'A', 'C', 'G', 'T', 'N', 'R', 'Y', 'K', 'M', 'S', 'W', 'B', 'D', 'H', 'V', 0};

// the 28 symmetric, non-transitive IUPAC equalities plus identity (specimux_amd/constants.py IUPAC_EQUIV)
static bool iupac_eq(unsigned char a, unsigned char b) {
    if (a == b) return true;
    static const char *pairs[] = {"YC", "YT", "RA", "RG", "NA", "NC", "NG", "NT", "WA", "WT", "MA", "MC", "SC", "SG",
                                  "KG", "KT", "BC", "BG", "BT", "DA", "DG", "DT", "HA", "HC", "HT", "VA", "VC", "VG"};
    for (const char *p : pairs)
        if (((unsigned char)p[0] == a && (unsigned char)p[1] == b) || ((unsigned char)p[0] == b && (unsigned char)p[1] == a)) return true;
    return false;
}

static int code_of(unsigned char c) {
    for (int i = 0; i < 15; i++)
        if ((unsigned char)kCodes[i] == c) return i;
    return 15;
}

// what a read byte is to a pattern letter: a byte outside the 15 letters matches nothing
static bool cell_eq(unsigned char p, unsigned char t) { return code_of(t) != 15 && iupac_eq(p, t); }

struct Pat {
    Seq s;
    int k;
};

// D(c) for every column c: the last row of the HW DP (row 0 is 0 everywhere)
static std::vector<int> last_row(const Seq &p, const Seq &t) {
    const int m = (int)p.size(), n = (int)t.size();
    std::vector<int> col(m + 1), out(n);
    for (int i = 0; i <= m; i++) col[i] = i;
    for (int j = 0; j < n; j++) {
        int diag = 0;
        for (int i = 1; i <= m; i++) {
            const int up = col[i - 1] + 1, left = col[i] + 1, sub = diag + (cell_eq((unsigned char)p[i - 1], (unsigned char)t[j]) ? 0 : 1);
            diag = col[i];
            col[i] = std::min(std::min(up, left), sub);
        }
        out[j] = col[m];
    }
    return out;
}

struct Out {
    std::vector<uint8_t> nhit;
    std::vector<int8_t> hd;
    std::vector<int32_t> he;
    bool operator==(const Out &o) const { return nhit == o.nhit && hd == o.hd && he == o.he; }
};

// the definition, over the whole read
static void ref_hits(const std::vector<int> &D, int k, int margin, int H, uint8_t *nhit, int8_t *hd, int32_t *he, long long *runs) {
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

// A call's patterns as the host driver lays them out: split by word width, passes of G, match words [pass][code][G]
struct Panel {
    std::vector<Pat> pats;
    std::vector<int> idx[2];
    int G[2] = {4, 4}, npass[2] = {0, 0}, lead = 1;
    std::vector<uint64_t> peq[2];   // class 0 holds 32-bit words (two per element), class 1 64-bit words
    std::vector<int> tab[2];        // pm, pk, jmap: npass * G each
    unsigned char lut[256];

    explicit Panel(const std::vector<Pat> &p) : pats(p) {
        for (int c = 0; c < 256; c++) lut[c] = (unsigned char)code_of((unsigned char)c);
        for (int j = 0; j < (int)pats.size(); j++) {
            lead = std::max(lead, (int)pats[j].s.size() + pats[j].k);
            idx[pats[j].s.size() > 32 ? 1 : 0].push_back(j);
        }
        for (int cls = 0; cls < 2; cls++) {
            if (idx[cls].empty()) continue;
            G[cls] = idx[cls].size() <= 4 ? 4 : 8;
            npass[cls] = (int)((idx[cls].size() + G[cls] - 1) / G[cls]);
            const size_t slots = (size_t)npass[cls] * G[cls];
            tab[cls].assign(3 * slots, -1);
            peq[cls].assign(slots * 16, 0);
            uint32_t *w32 = reinterpret_cast<uint32_t *>(peq[cls].data());
            for (size_t s = 0; s < slots; s++) {
                tab[cls][s] = 1;
                if (s >= idx[cls].size()) continue;
                const Pat &P = pats[idx[cls][s]];
                tab[cls][s] = (int)P.s.size();
                tab[cls][slots + s] = P.k;
                tab[cls][2 * slots + s] = idx[cls][s];
                for (int c = 0; c < 15; c++)
                    for (size_t i = 0; i < P.s.size(); i++)
                        if (iupac_eq((unsigned char)P.s[i], (unsigned char)kCodes[c])) {
                            const size_t at = ((s / G[cls]) * 16 + c) * G[cls] + s % G[cls];
                            if (cls == 0) w32[at] |= 1u << i;
                            else peq[cls][at] |= 1ull << i;
                        }
            }
        }
    }
};

struct Sim {
    std::mt19937_64 rng;
    long long cases = 0, scans = 0, units = 0, mismatches = 0;
    std::map<std::string, long long> count;
    std::vector<mine_u4> buf;
    std::vector<uint32_t> recs;

    explicit Sim(uint64_t seed) : rng(seed) {}

    template <typename W>
    void scan_class(const Panel &P, int cls, const unsigned char *lut, uint64_t roff, int n, int margin, int PL, int H, int npieces) {
        const std::vector<int> &idx = P.idx[cls];
        if (idx.empty()) return;
        const int G = P.G[cls], Q = (int)P.pats.size(), RW = inner_rec_words(H);
        for (int pass = 0; pass < P.npass[cls]; pass++) {
            const W *peq = reinterpret_cast<const W *>(P.peq[cls].data()) + (size_t)pass * 16 * G;
            const int *pm = P.tab[cls].data() + (size_t)pass * G, *pk = pm + (size_t)P.npass[cls] * G, *jm = pk + (size_t)P.npass[cls] * G;
            for (int piece = 0; piece < npieces; piece++) {
                uint32_t *rec_unit = recs.data() + (size_t)piece * Q * RW;
                if (G == 4) inner_scan_piece<W, 4>(peq, lut, pm, pk, jm, buf.data(), roff, n, margin, PL, P.lead, piece, H, rec_unit);
                else inner_scan_piece<W, 8>(peq, lut, pm, pk, jm, buf.data(), roff, n, margin, PL, P.lead, piece, H, rec_unit);
                units++;
            }
        }
        count[cls == 0 ? "class_32" : "class_64"] += (long long)idx.size();
    }

    // one call of the scan as the host driver and the kernels would run it, at piece length PL
    void scan_core(const Panel &P, const Seq &read, int margin, int H, int PL, uint64_t roff, Out *out) {
        const int Q = (int)P.pats.size(), n = (int)read.size(), RW = inner_rec_words(H);
        // the read where the driver puts it: at byte roff of a buffer of 16-byte words, junk on both sides
        buf.assign((roff + (uint64_t)n) / 16 + 2, mine_u4{0, 0, 0, 0});
        unsigned char *b = reinterpret_cast<unsigned char *>(buf.data());
        for (size_t i = 0; i < buf.size() * 16; i += 8) { const uint64_t junk = rng(); memcpy(b + i, &junk, 8); }
        memcpy(b + roff, read.data(), (size_t)n);
        const int npieces = n > 2 * margin ? (n - 2 * margin + PL - 1) / PL : 0;
        recs.assign((size_t)npieces * Q * RW, 0xdeadbeefu);   // the kernel's records start as junk too
        scan_class<uint32_t>(P, 0, P.lut, roff, n, margin, PL, H, npieces);
        scan_class<uint64_t>(P, 1, P.lut, roff, n, margin, PL, H, npieces);
        out->nhit.assign(Q, 0);
        out->hd.assign((size_t)Q * H, 0);
        out->he.assign((size_t)Q * H, 0);
        for (int j = 0; j < Q; j++)
            inner_merge(recs.data(), 0, npieces, Q, j, H, margin, PL, &out->nhit[j], &out->hd[(size_t)j * H], &out->he[(size_t)j * H]);
        scans++;
    }

    void ref(const Panel &P, const std::vector<std::vector<int>> &D, int margin, int H, Out *out, long long *runs) {
        const std::vector<Pat> &pats = P.pats;
        const int Q = (int)pats.size();
        out->nhit.assign(Q, 0);
        out->hd.assign((size_t)Q * H, 0);
        out->he.assign((size_t)Q * H, 0);
        for (int j = 0; j < Q; j++) ref_hits(D[j], pats[j].k, margin, H, &out->nhit[j], &out->hd[(size_t)j * H], &out->he[(size_t)j * H], runs);
    }

    void compare(const Out &want, const Out &got, const char *what, const Seq &read, int margin, int H, int PL) {
        if (want == got) return;
        if (mismatches < 10) {
            fprintf(stderr, "MISMATCH %s n=%zu margin=%d H=%d PL=%d read=%.60s\n", what, read.size(), margin, H, PL, read.c_str());
            for (size_t j = 0; j < want.nhit.size(); j++)
                if (want.nhit[j] != got.nhit[j] || memcmp(&want.hd[j * H], &got.hd[j * H], H) || memcmp(&want.he[j * H], &got.he[j * H], 4 * H))
                    fprintf(stderr, "  pattern %zu: want n=%d d0=%d e0=%d, got n=%d d0=%d e0=%d\n", j, want.nhit[j], want.hd[j * H],
                            want.he[j * H], got.nhit[j], got.hd[j * H], got.he[j * H]);
        }
        mismatches++;
    }
};

static void all_strings(const char *alphabet, int len, std::vector<Seq> *out) {
    const int a = (int)strlen(alphabet);
    long long total = 1;
    for (int i = 0; i < len; i++) total *= a;
    for (long long v = 0; v < total; v++) {
        Seq s(len, ' ');
        long long x = v;
        for (int i = 0; i < len; i++) { s[i] = alphabet[x % a]; x /= a; }
        out->push_back(s);
    }
}

static int run_exhaustive() {
    std::vector<Pat> pats;   // every (pattern, valid k)
    for (int m = 1; m <= 5; m++) {
        std::vector<Seq> ps;
        all_strings("AC", m, &ps);
        for (const Seq &p : ps)
            for (int k = 0; k < m; k++) pats.push_back(Pat{p, k});
    }
    std::vector<Seq> reads;
    for (int n = 0; n <= 9; n++) all_strings("ACN", n, &reads);
    // calls of up to 43 (pattern, k) slots: several passes of 8 per call, as a panel would
    std::vector<Panel> groups;
    for (size_t i = 0; i < pats.size(); i += 43)
        groups.emplace_back(std::vector<Pat>(pats.begin() + i, pats.begin() + std::min(pats.size(), i + 43)));
    const int T = (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    std::vector<Sim> sims;
    std::vector<long long> runs(T, 0);
    for (int t = 0; t < T; t++) sims.emplace_back(1 + t);
    auto work = [&](int t) {
        Sim &sim = sims[t];
        for (size_t ri = t; ri < reads.size(); ri += T) {
            const Seq &read = reads[ri];
            for (const Panel &grp : groups) {
                std::vector<std::vector<int>> D;
                for (const Pat &P : grp.pats) D.push_back(last_row(P.s, read));
                for (int margin = 0; margin <= 3; margin++) {
                    for (int H : {1, 3}) {
                        Out want, got;
                        sim.ref(grp, D, margin, H, &want, &runs[t]);
                        // the kernel's piece length for these patterns and, for every fourth read, pieces of 1-3 columns
                        // (every run longer than that crosses a boundary)
                        const int pls[2] = {inner_piece_len(grp.lead), H == 1 ? 2 : (margin & 1 ? 1 : 3)};
                        for (int PL : pls) {
                            if (PL != pls[0] && (ri % 4 != 0 || (int)read.size() <= 2 * margin)) continue;
                            sim.scan_core(grp, read, margin, H, PL, (uint64_t)(read.size() * 7 + margin) % 23, &got);
                            sim.compare(want, got, "exhaustive", read, margin, H, PL);
                        }
                        sim.cases += (long long)grp.pats.size();
                    }
                }
            }
        }
    };
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) th.emplace_back(work, t);
    for (auto &x : th) x.join();
    long long cases = 0, scans = 0, units = 0, nruns = 0, mismatches = 0;
    for (int t = 0; t < T; t++) {
        cases += sims[t].cases; scans += sims[t].scans; units += sims[t].units; nruns += runs[t]; mismatches += sims[t].mismatches;
    }
    printf("patterns %zu\nreads %zu\ncases %lld\nscans %lld\nunits %lld\nruns %lld\n", pats.size(), reads.size(), cases, scans, units, nruns);
    printf("%lld mismatches\n", mismatches);
    return mismatches ? 1 : 0;
}

// ---- structured random cases
static Seq random_seq(std::mt19937_64 &rng, int n, const char *alphabet) {
    const int a = (int)strlen(alphabet);
    Seq s(n, ' ');
    for (int i = 0; i < n; i++) s[i] = alphabet[rng() % a];
    return s;
}

// a concrete read-side copy of a pattern: degenerate letters resolved to one of the bases they equal
static Seq concrete(std::mt19937_64 &rng, const Seq &p) {
    Seq s = p;
    for (char &c : s) {
        char pick[4];
        int np = 0;
        for (char b : {'A', 'C', 'G', 'T'})
            if (iupac_eq((unsigned char)c, (unsigned char)b)) pick[np++] = b;
        c = pick[rng() % np];
    }
    return s;
}

// e random edits (substitution to a letter that differs, insertion, deletion)
static Seq edited(std::mt19937_64 &rng, Seq s, int e) {
    for (int i = 0; i < e; i++) {
        const int kind = s.size() > 1 ? (int)(rng() % 3) : (int)(rng() % 2);
        const size_t at = rng() % s.size();
        const char b = "ACGT"[rng() % 4];
        if (kind == 0) s[at] = s[at] == b ? (b == 'A' ? 'C' : 'A') : b;
        else if (kind == 1) s.insert(s.begin() + at, b);
        else s.erase(s.begin() + at);
    }
    return s;
}

static std::string hex(const Seq &s) {
    static const char *d = "0123456789abcdef";
    std::string o;
    for (unsigned char c : s) { o += d[c >> 4]; o += d[c & 15]; }
    return o.empty() ? "-" : o;
}

static int run_random(uint64_t seed) {
    Sim sim(seed);
    std::mt19937_64 &rng = sim.rng;
    FILE *fo = fopen("oracle_sample.txt", "w");
    if (!fo) { perror("oracle_sample.txt"); return 2; }
    long long runs = 0, oracle_sample = 0;
    const int ms[8] = {1, 19, 22, 31, 32, 33, 63, 64};
    // every piece length the kernel can choose, and two it cannot
    const int pls[6] = {64, 128, 256, 512, 37, 100};
    for (int rep = 0; rep < 48; rep++) {
        // a panel: every length once or twice, thresholds from 0 to m - 1, some letters degenerate
        std::vector<Pat> pats;
        for (int m : ms) {
            for (int copy = 0; copy < 1 + (int)(rng() % 2); copy++) {
                Seq p = random_seq(rng, m, "ACGT");
                for (char &c : p)
                    if (rng() % 8 == 0) c = "NRYKMSWBDHV"[rng() % 11];
                const int kind = (int)(rng() % 4);
                const int k = kind == 0 ? 0 : kind == 1 ? m - 1 : (int)(rng() % m) / (kind == 2 ? 1 : 4);
                pats.push_back(Pat{p, std::min(k, m - 1)});
            }
        }
        std::shuffle(pats.begin(), pats.end(), rng);
        const Panel panel(pats);
        const int Q = (int)pats.size();
        for (int rd = 0; rd < 6; rd++) {
            const int margin = (int)(rng() % 4 == 0 ? rng() % 5 : 40 + rng() % 60);
            Seq read = random_seq(rng, 300 + (int)(rng() % 1200), "ACGT");
            const int n = (int)read.size();
            // plant copies: at distance exactly k and k + 1 (checked by DP on the copy), two back to back (their runs touch for a large enough k) and two with one
            // base between them, anywhere in the read (the windows and their edges included)
            for (int pl = 0; pl < 10; pl++) {
                const Pat &P = pats[rng() % Q];
                const int kind = pl % 5;
                Seq ins;
                const char *name;
                if (kind < 2) {
                    // k or k + 1 random edits: edits can cancel or fall under a degenerate letter, so the copy's own best
                    // distance is checked (a few attempts) and decides which counter it goes to
                    int best = -1;
                    for (int attempt = 0; attempt < 6 && best != P.k + kind; attempt++) {
                        ins = edited(rng, concrete(rng, P.s), P.k + kind);
                        const std::vector<int> d = ins.empty() ? std::vector<int>() : last_row(P.s, ins);
                        best = d.empty() ? (int)P.s.size() : *std::min_element(d.begin(), d.end());
                    }
                    name = best == P.k ? "kind_at_k" : best == P.k + 1 ? "kind_at_k_plus_1" : "kind_edited_other";
                }
                else if (kind == 2) { ins = concrete(rng, P.s) + concrete(rng, P.s); name = "kind_touching"; }
                else if (kind == 3) { ins = concrete(rng, P.s) + "ACGT"[rng() % 4] + concrete(rng, P.s); name = "kind_one_apart"; }
                else { ins = concrete(rng, P.s); name = "kind_exact"; }
                if ((int)ins.size() >= n) continue;
                const size_t at = rng() % (n - ins.size());
                read.replace(at, ins.size(), ins);
                sim.count[name]++;
            }
            // read bytes the code map has to get right: N and R match what they equal, lower case and 0xFF nothing
            for (int i = 0; i < 6; i++) read[rng() % n] = "NRacgn\xff"[rng() % 7];
            std::vector<std::vector<int>> D;
            for (const Pat &P : pats) D.push_back(last_row(P.s, read));
            const int H = (int)(1 + rng() % 8);
            Out want, got;
            sim.ref(panel, D, margin, H, &want, &runs);
            for (int j = 0; j < Q; j++) {
                if (want.nhit[j] > H) sim.count["more_than_H"]++;
                // runs that cross a boundary of the kernel's own grid
                const int PLk = 128;
                for (int c = margin + PLk; c < n - margin; c += PLk)
                    if (D[j][c] <= pats[j].k && D[j][c - 1] <= pats[j].k) sim.count["runs_across_boundary"]++;
            }
            for (int PL : pls) {
                sim.scan_core(panel, read, margin, H, PL, rng() % 64, &got);
                sim.compare(want, got, "random", read, margin, H, PL);
                sim.count["pl_" + std::to_string(PL)]++;
            }
            sim.cases += Q;
            // the DP itself against the suite's oracle: best distance over a prefix of the read and its first end
            if (rd == 0) {
                for (int s = 0; s < 4; s++) {
                    const int j = (int)(rng() % Q);
                    const int cut = std::min(n, 60 + (int)(rng() % 200));
                    int best = 1 << 30, end = -1;
                    for (int c = 0; c < cut; c++)
                        if (D[j][c] < best) { best = D[j][c]; end = c; }
                    fprintf(fo, "%s %s %d %d\n", hex(pats[j].s).c_str(), hex(read.substr(0, cut)).c_str(), best, end);
                    oracle_sample++;
                }
            }
        }
    }
    fclose(fo);
    printf("cases %lld\nscans %lld\nunits %lld\nruns %lld\noracle_sample %lld\n", sim.cases, sim.scans, sim.units, runs, oracle_sample);
    for (const auto &kv : sim.count) printf("%s %lld\n", kv.first.c_str(), kv.second);
    printf("%lld mismatches\n", sim.mismatches);
    return sim.mismatches ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "exhaustive")) return run_exhaustive();
    if (argc >= 3 && !strcmp(argv[1], "random")) return run_random(strtoull(argv[2], nullptr, 10));
    fprintf(stderr, "usage: inner_sim exhaustive | random <seed>\n");
    return 2;
}
