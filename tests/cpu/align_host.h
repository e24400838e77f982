// The alignment kernels' lane bodies (specimux_amd/csrc/smx_align_lane.h) compiled for the host, a plain full-matrix
// reference written from oracle/edlib_semantics.py's align_py, and the checkers and case families that
// tests/cpu/align_sim.cpp and tests/asan/align_driver.cpp share.  Every buffer a lane body indexes is a heap vector of
// exactly the size smx_align / smx_align_batch (smx_calls.cpp) allocate: tlen bytes of scores and tlen starts for one
// alignment, toff[n] bytes of scores and n * cap locations for a batch.
#ifndef ALIGN_HOST_H
#define ALIGN_HOST_H
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <thread>
#include <vector>

// smx_align_core.h is device code; the host build defines its qualifiers away and compiles the same lines
#define __device__
#define __forceinline__ inline
#include "smx_align_lane.h"
#undef __device__
#undef __forceinline__

namespace align_host {
typedef unsigned long long u64;

struct Stats {
    long long mismatches = 0;
    std::map<std::string, long long> count;
    void bad(const char *what, const std::string &q, const std::string &t, int mode, int k, long long a = 0, long long b = 0) {
        if (++mismatches <= 20)
            printf("MISMATCH %s q=%s tlen=%zu t=%.40s mode=%d k=%d %lld %lld\n", what, q.c_str(), t.size(), t.c_str(), mode, k, a, b);
    }
};

// ---- the alphabet, twice.  The Peq tables come from base sets (a letter is the set of bases it stands for; two different
// letters are equal when exactly one of them is a single base and the other's set holds it); the reference compares
// letters through the list of 28 pairs.  check_alphabet holds the two against each other.
static const char kLetters[16] = "ACGTNRYKMSWBDHV";   // the order of smx::kCodeChars; code 15 = any other byte
inline int code_of(unsigned char c) {
    for (int i = 0; i < 15; i++)
        if ((unsigned char)kLetters[i] == c) return i;
    return 15;
}
inline unsigned base_set(char c) {
    switch (c) {
        case 'A': return 1; case 'C': return 2; case 'G': return 4; case 'T': return 8;
        case 'R': return 1 | 4; case 'Y': return 2 | 8; case 'K': return 4 | 8; case 'M': return 1 | 2;
        case 'S': return 2 | 4; case 'W': return 1 | 8; case 'B': return 2 | 4 | 8; case 'D': return 1 | 4 | 8;
        case 'H': return 1 | 2 | 8; case 'V': return 1 | 2 | 4; case 'N': return 15;
        default: return 0;
    }
}
inline bool set_eq(char a, char b) {
    const unsigned sa = base_set(a), sb = base_set(b);
    if (!sa || !sb) return false;
    if (a == b) return true;
    const bool one_a = (sa & (sa - 1)) == 0, one_b = (sb & (sb - 1)) == 0;
    return one_a != one_b && (sa & sb) != 0;
}
struct PairTable {   // edlib_semantics.eq: equal bytes, or one of the 28 pairs in either order
    bool eq[256][256];
    PairTable() {
        memset(eq, 0, sizeof eq);
        for (int c = 0; c < 256; c++) eq[c][c] = true;
        const char *pairs = "YC YT RA RG NA NC NG NT WA WT MA MC SC SG KG KT BC BG BT DA DG DT HA HC HT VA VC VG";
        for (const char *p = pairs; *p; p += (p[2] ? 3 : 2)) eq[(int)p[0]][(int)p[1]] = eq[(int)p[1]][(int)p[0]] = true;
    }
};
inline bool pair_eq(char a, char b) {
    static const PairTable table;
    return table.eq[(unsigned char)a][(unsigned char)b];
}
// bit i of peq16[c] = the query's letter i equals the letter of code c; code 15 never matches.  false: a letter outside
// the alphabet, which smx_align refuses
inline bool build_peq(const std::string &q, u64 *peq16) {
    for (int c = 0; c < 16; c++) peq16[c] = 0;
    for (size_t i = 0; i < q.size(); i++) {
        if (code_of((unsigned char)q[i]) == 15) return false;
        for (int c = 0; c < 15; c++)
            if (set_eq(q[i], kLetters[c])) peq16[c] |= 1ull << i;
    }
    return true;
}
inline void check_alphabet(Stats &S) {
    long long off_diagonal = 0;
    for (int a = 0; a < 15; a++)
        for (int b = 0; b < 15; b++) {
            if (set_eq(kLetters[a], kLetters[b]) != pair_eq(kLetters[a], kLetters[b])) S.bad("alphabet", "", "", a, b);
            off_diagonal += a != b && pair_eq(kLetters[a], kLetters[b]);
        }
    S.count["iupac_pairs"] = off_diagonal / 2;
    u64 peq[16];
    std::string all(kLetters, 15);
    if (!build_peq(all, peq) || peq[15] != 0 || build_peq("AxA", peq) || build_peq("a", peq)) S.bad("peq", all, "", 0, 0);
}

// ---- the reference: edlib_semantics.align_py.  Last row of the full matrix of q against t; shw: D[0][j] = j, else 0
inline std::vector<int> last_row(const std::string &q, const std::string &t, bool shw) {
    const int m = (int)q.size(), n = (int)t.size();
    static thread_local std::vector<int> D;   // the matrix, kept between calls: millions of them are tiny
    D.resize((size_t)(m + 1) * (n + 1));
    auto at = [&](int i, int j) -> int & { return D[(size_t)i * (n + 1) + j]; };
    for (int i = 0; i <= m; i++) at(i, 0) = i;
    for (int j = 1; j <= n; j++) at(0, j) = shw ? j : 0;
    for (int j = 1; j <= n; j++)
        for (int i = 1; i <= m; i++)
            at(i, j) = std::min(std::min(at(i - 1, j - 1) + (pair_eq(q[i - 1], t[j - 1]) ? 0 : 1), at(i, j - 1) + 1), at(i - 1, j) + 1);
    return std::vector<int>(D.begin() + (size_t)m * (n + 1), D.begin() + (size_t)(m + 1) * (n + 1));
}

struct Ref {
    int best = 0;                  // the minimum of the last row, whatever k is
    std::vector<int> row;          // the last row, [0..n]
    std::vector<int> starts, ends; // every optimal end in ascending order, with its start
};
// mode 0 = HW, 1 = SHW.  The start rule: the smallest start s with NW(q, t[s..e]) == best.  NW of a piece of c letters
// costs at least c - m, so only pieces of at most m + best letters are tried (align_py tries them all).
inline Ref ref_align(const std::string &q, const std::string &t, int mode) {
    const int m = (int)q.size(), n = (int)t.size();
    Ref r;
    r.row = last_row(q, t, mode == 1);
    r.best = *std::min_element(r.row.begin() + 1, r.row.end());
    const std::string rq(q.rbegin(), q.rend());
    for (int j = 1; j <= n; j++) {
        if (r.row[j] != r.best) continue;
        const int e = j - 1;
        int s = 0;
        if (mode == 0) {
            const int L = std::min(e + 1, m + r.best);
            std::string rt(t.begin() + (e + 1 - L), t.begin() + (e + 1));
            std::reverse(rt.begin(), rt.end());
            const std::vector<int> rl = last_row(rq, rt, true);
            int p = 0;
            for (int c = 1; c <= L; c++)
                if (rl[c] == r.best) p = c - 1;
            s = e - p;
        }
        r.starts.push_back(s);
        r.ends.push_back(e);
    }
    return r;
}
// a case whose untrimmed SHW last row holds a column with a score >= 256 that equals best in its low byte
inline bool wrap_witness(const Ref &r) {
    for (size_t j = 1; j < r.row.size(); j++)
        if (r.row[j] >= 256 && (r.row[j] - r.best) % 256 == 0) return true;
    return false;
}

static const int SENTINEL = 0x5EADBEEF;

struct Query {
    std::string q;
    u64 peq[32];
    bool ok;
    explicit Query(const std::string &s) : q(s) {
        ok = build_peq(s, peq) && build_peq(std::string(s.rbegin(), s.rend()), peq + 16);
    }
};
struct Target {   // a target with the buffers smx_align gives it: tlen codes, tlen score bytes, tlen starts
    std::string t;
    std::vector<unsigned char> codes, flag;
    std::vector<int> starts;
    explicit Target(const std::string &s) : t(s), codes(s.size()), flag(s.size()), starts(s.size()) {
        for (size_t i = 0; i < s.size(); i++) codes[i] = (unsigned char)code_of((unsigned char)s[i]);
    }
};
struct OutPool {   // location buffers of exactly cap ints, kept by cap
    std::map<int, std::pair<std::vector<int>, std::vector<int>>> bufs;
    std::pair<std::vector<int>, std::vector<int>> &get(int cap) {
        auto it = bufs.find(cap);
        if (it == bufs.end()) it = bufs.emplace(cap, std::make_pair(std::vector<int>(cap), std::vector<int>(cap))).first;
        return it->second;
    }
};

// smx_align as smx_calls.cpp runs it: the lane over the target's buffers, then align_collect for every cap of `caps`
inline void check_single(Stats &S, const Query &Q, Target &T, int mode, int k, const Ref &r, std::initializer_list<int> caps, OutPool &pool) {
    const int n = (int)T.t.size(), want = r.best > k ? -1 : r.best, want_n = want < 0 ? 0 : (int)r.ends.size();
    std::fill(T.flag.begin(), T.flag.end(), (unsigned char)0xA5);
    std::fill(T.starts.begin(), T.starts.end(), SENTINEL);
    int dist = SENTINEL;
    smx::align_lane(Q.peq, Q.peq + 16, (int)Q.q.size(), T.codes.data(), n, k, mode, &dist, T.flag.data(), T.starts.data());
    if (dist != want) { S.bad("single dist", Q.q, T.t, mode, k, dist, want); return; }
    for (int cap : caps) {
        auto &out = pool.get(cap);
        std::fill(out.first.begin(), out.first.end(), SENTINEL);
        std::fill(out.second.begin(), out.second.end(), SENTINEL);
        const int cnt = smx::align_collect(dist, T.flag.data(), T.starts.data(), n, cap ? out.first.data() : nullptr,
                                           cap ? out.second.data() : nullptr, cap);
        if (cnt != want_n) { S.bad("single nloc", Q.q, T.t, mode, k, cnt, want_n); return; }
        for (int x = 0; x < cap; x++) {
            const int ws = x < want_n ? r.starts[x] : SENTINEL, we = x < want_n ? r.ends[x] : SENTINEL;
            if (out.first[x] != ws || out.second[x] != we) { S.bad("single location", Q.q, T.t, mode, k, x, out.second[x]); break; }
        }
    }
}

struct Item {   // one alignment of a batch
    unsigned qi;
    const Target *T;
    int k, mode;
    const Ref *r;
};
// smx_align_batch as smx_calls.cpp runs it: one launch of items.size() lanes with location buffers of n * cap ints (none
// where cap == 0) and a score workspace of toff[n] bytes that holds `fill`, as a grow-only workspace holds what the
// call before left there
inline void check_batch(Stats &S, const std::vector<const Query *> &queries, const std::vector<Item> &items, unsigned cap, unsigned char fill) {
    const unsigned n = (unsigned)items.size();
    std::vector<u64> q_peq(queries.size() * 32), toff(n + 1, 0);
    std::vector<int> q_len(queries.size()), kk(n), out_dist(n, SENTINEL), out_nloc(n, SENTINEL);
    std::vector<unsigned> qidx(n);
    std::vector<unsigned char> modes(n);
    for (size_t q = 0; q < queries.size(); q++) {
        memcpy(&q_peq[q * 32], queries[q]->peq, sizeof queries[q]->peq);
        q_len[q] = (int)queries[q]->q.size();
    }
    for (unsigned i = 0; i < n; i++) {
        toff[i + 1] = toff[i] + items[i].T->t.size();
        qidx[i] = items[i].qi, kk[i] = items[i].k, modes[i] = (unsigned char)items[i].mode;
    }
    std::vector<unsigned char> tcodes(toff[n]), ws(toff[n], fill);
    for (unsigned i = 0; i < n; i++) std::copy(items[i].T->codes.begin(), items[i].T->codes.end(), tcodes.begin() + toff[i]);
    std::vector<int> starts((size_t)n * cap, SENTINEL), ends((size_t)n * cap, SENTINEL);
    for (unsigned i = 0; i < n; i++)
        smx::align_batch_lane(i, q_peq.data(), q_len.data(), qidx.data(), tcodes.data(), toff.data(), kk.data(), modes.data(),
                              ws.data(), out_dist.data(), out_nloc.data(), cap ? starts.data() : nullptr,
                              cap ? ends.data() : nullptr, cap);
    S.count["batch_launches"]++;
    if (cap == 0) S.count["cap_zero_launches"]++;
    if (fill != 0) S.count["dirty_workspace_launches"]++;
    long long below = 0;
    for (unsigned i = 0; i < n; i++) {
        const Item &I = items[i];
        const Ref &r = *I.r;
        const std::string &q = queries[I.qi]->q;
        const int want = r.best > I.k ? -1 : r.best, want_n = want < 0 ? 0 : (int)r.ends.size();
        if (out_dist[i] != want) { S.bad("batch dist", q, I.T->t, I.mode, I.k, out_dist[i], want); continue; }
        if (out_nloc[i] != want_n) { S.bad("batch nloc", q, I.T->t, I.mode, I.k, out_nloc[i], want_n); continue; }
        below += (unsigned)want_n > cap;
        for (unsigned x = 0; x < cap; x++) {   // the first min(nloc, cap) locations; the slots behind them are left alone
            const int w_s = (int)x < want_n ? r.starts[x] : SENTINEL, w_e = (int)x < want_n ? r.ends[x] : SENTINEL;
            if (starts[(size_t)i * cap + x] != w_s || ends[(size_t)i * cap + x] != w_e) { S.bad("batch location", q, I.T->t, I.mode, I.k, i, x); break; }
        }
    }
    S.count["cap_below_nloc"] += below;
}

// ---- the wrap families: f(query, target, k, full_prefix) for every case; both entries and both modes are the caller's
static const int kWrapM[8] = {1, 2, 6, 7, 20, 58, 63, 64};
static const int kWrapK[7] = {0, -1 /* m - 1 */, -2 /* m */, 200, 249, 250, 1000};   // 1000: the single call only
inline std::string wrap_query(int m) {   // over A, G and one R: `C` and `x` match none of its letters
    std::mt19937 rng(1000 + m);
    std::string q(m, 'A');
    for (char &c : q) c = "AG"[rng() % 2];
    if (m >= 6) q[m / 2] = 'R';
    return q;
}
template <class F> void wrap_cases(F f) {
    for (int m : kWrapM) {
        const std::string q = wrap_query(m);
        for (int kc : kWrapK) {
            const int k = kc == -1 ? m - 1 : kc == -2 ? m : kc;
            const int lens[10] = {m + k - 1, m + k, m + k + 1, 255, 256, 257, m + 255, m + 256, 600, 1000};
            for (int n : lens) {
                if (n < 1) continue;
                const char fill = (n + k) % 2 ? 'C' : 'x';
                std::mt19937 rng(m * 7919 + k * 31 + n);
                // the query, then filler: with n >= m + 256 column m + 256 costs 256 and column m costs 0
                std::string t = q.substr(0, std::min(m, n)) + std::string(n - std::min(m, n), fill);
                f(q, t, k, n >= m + 256);
                // half the query, then filler
                t = q.substr(0, std::min(m / 2, n)) + std::string(n - std::min(m / 2, n), fill);
                f(q, t, k, false);
                // no matching letter
                for (int i = 0; i < n; i++) t[i] = i % 3 == 0 ? 'x' : 'C';
                f(q, t, k, false);
                // two letters, one of which the query holds
                for (int i = 0; i < n; i++) t[i] = "AC"[rng() % 2];
                f(q, t, k, false);
            }
        }
    }
}
// the wrap families through both lane bodies: every case alone, and the cases with k <= 250 in launches of up to 64
inline void run_wrap(Stats &S) {
    OutPool pool;
    std::vector<Query *> qs;
    std::vector<Target *> ts;
    std::vector<Ref *> refs;
    std::vector<Item> items;
    std::vector<const Query *> queries;
    wrap_cases([&](const std::string &q, const std::string &t, int k, bool full_prefix) {
        if (qs.empty() || qs.back()->q != q) { qs.push_back(new Query(q)); queries.push_back(qs.back()); }
        ts.push_back(new Target(t));
        for (int mode = 0; mode < 2; mode++) {
            Ref *r = new Ref(ref_align(q, t, mode));
            refs.push_back(r);
            const int nloc = r->best > k ? 0 : (int)r->ends.size();
            check_single(S, *qs.back(), *ts.back(), mode, k, *r, {0, 1, nloc}, pool);
            S.count["single_cases"]++;
            if (mode == 1) {
                if (full_prefix) S.count["full_prefix_cases"]++;
                if (wrap_witness(*r)) S.count["wrap_witnesses"]++;
                if (full_prefix && !wrap_witness(*r)) S.bad("a full prefix is no witness", q, t, mode, k);
            }
            if (k >= (int)q.size()) S.count[mode ? "k_ge_m_shw" : "k_ge_m_hw"]++;
            if (k <= 250) items.push_back(Item{(unsigned)qs.size() - 1, ts.back(), k, mode, r});
        }
    });
    for (size_t at = 0; at < items.size(); at += 64) {
        const std::vector<Item> part(items.begin() + at, items.begin() + std::min(items.size(), at + 64));
        int most = 0;
        for (const Item &I : part) most = std::max(most, I.r->best > I.k ? 0 : (int)I.r->ends.size());
        for (unsigned cap : {0u, 1u, (unsigned)std::max(most - 1, 0), (unsigned)most})
            check_batch(S, queries, part, cap, (unsigned char)(at / 64 % 2 ? 0xFF : 0));
        S.count["batch_cases"] += (long long)part.size();
    }
    for (Query *p : qs) delete p;
    for (Target *p : ts) delete p;
    for (Ref *p : refs) delete p;
}

// ---- the exhaustive set: every query of 1..4 letters and every target of 1..7 letters over {A, C, N, x}, both modes,
// k = 0..5, cap in {0, 1, nloc}.  A query that holds `x` is one smx_align refuses: build_peq must say so, and no lane runs
inline void exhaustive_part(Stats &S, int part, int parts) {   // the part-th of every `parts` queries that are not refused
    const char letters[4] = {'A', 'C', 'N', 'x'};
    std::vector<Target *> ts;
    for (int n = 1; n <= 7; n++)
        for (int v = 0; v < 1 << (2 * n); v++) {
            std::string t(n, 'A');
            for (int i = 0; i < n; i++) t[i] = letters[(v >> (2 * i)) & 3];
            ts.push_back(new Target(t));
        }
    OutPool pool;
    long long cases = 0, k_ge_m[2] = {0, 0}, several = 0, above = 0;
    int at = 0;
    for (int m = 1; m <= 4; m++)
        for (int v = 0; v < 1 << (2 * m); v++) {
            std::string q(m, 'A');
            for (int i = 0; i < m; i++) q[i] = letters[(v >> (2 * i)) & 3];
            const Query Q(q);
            if (!Q.ok && part == 0) S.count["queries_refused"]++;
            if (Q.ok != (q.find('x') == std::string::npos)) S.bad("query refusal", q, "", 0, 0);
            if (!Q.ok || at++ % parts != part) continue;
            S.count["queries"]++;
            const std::vector<const Query *> queries{&Q};
            for (int mode = 0; mode < 2; mode++) {
                std::vector<Ref> refs;
                refs.reserve(ts.size());
                for (Target *T : ts) refs.push_back(ref_align(q, T->t, mode));
                for (int k = 0; k <= 5; k++) {
                    std::vector<std::vector<Item>> by_nloc(8);
                    std::vector<Item> all;
                    all.reserve(ts.size());
                    for (size_t x = 0; x < ts.size(); x++) {
                        const int nloc = refs[x].best > k ? 0 : (int)refs[x].ends.size();
                        check_single(S, Q, *ts[x], mode, k, refs[x], {0, 1, nloc}, pool);
                        const Item I{0, ts[x], k, mode, &refs[x]};
                        all.push_back(I);
                        by_nloc[nloc].push_back(I);
                        cases++;
                        k_ge_m[mode] += k >= m;
                        several += nloc > 1;
                        above += nloc == 0;
                    }
                    check_batch(S, queries, all, 0, 0x00);
                    check_batch(S, queries, all, 1, 0xFF);
                    for (unsigned nloc = 2; nloc < by_nloc.size(); nloc++)   // cap == nloc (0 and 1 are the launches above)
                        if (!by_nloc[nloc].empty()) check_batch(S, queries, by_nloc[nloc], nloc, (unsigned char)(0x11 * nloc));
                }
            }
        }
    for (Target *p : ts) delete p;
    S.count["cases"] = cases, S.count["k_ge_m_hw"] = k_ge_m[0], S.count["k_ge_m_shw"] = k_ge_m[1];
    S.count["several_locations"] = several, S.count["above_k"] = above;
}
inline void run_exhaustive(Stats &S) {   // on up to eight threads, each with targets, buffers and counters of its own
    const int parts = (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    std::vector<Stats> stats(parts);
    std::vector<std::thread> threads;
    for (int p = 0; p < parts; p++) threads.emplace_back(exhaustive_part, std::ref(stats[p]), p, parts);
    for (std::thread &t : threads) t.join();
    for (const Stats &s : stats) {
        S.mismatches += s.mismatches;
        for (const auto &kv : s.count) S.count[kv.first] += kv.second;
    }
}

}  // namespace align_host
#endif
