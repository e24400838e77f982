// CPU simulation of the identify call (specimux_amd/csrc/smx_hits.hip): the host plan (smx_hits_plan.h) and the kernel
// as a host loop over the planned chunks (tests/cpu/hits_host.h: mine_pair and smx_hits_core.h called as the kernel calls
// them), checked against a plain O(mn) DP with edlib's HW semantics under the pair rule, reduced by a full sort.
// Built and run by tests/test_hits_cpu.py (g++, no GPU).
//
//   hits_sim <seed>      the scenarios of main, each with K = 1, 3 and 16; writes oracle_sample.txt in the cwd
//
// Prints "<counter> <value>" lines (the Python test asserts lower bounds on them) and "<n> mismatches".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "hits_host.h"

using namespace smx;
typedef std::string Seq;

static int dp_hw(const Seq &q, const Seq &t) {   // HW: D[i][0] = i, D[0][j] = 0, the minimum of the last row
    const int m = (int)q.size(), n = (int)t.size();
    std::vector<int> col(m + 1);
    for (int i = 0; i <= m; i++) col[i] = i;
    int best = col[m];
    for (int j = 0; j < n; j++) {
        int diag = col[0];
        col[0] = 0;
        const unsigned char c = (unsigned char)t[j];
        for (int i = 1; i <= m; i++) {
            const int up = col[i - 1] + 1, left = col[i] + 1, sub = diag + ((unsigned char)q[i - 1] == c ? 0 : 1);
            diag = col[i];
            col[i] = std::min(std::min(up, left), sub);
        }
        best = std::min(best, col[m]);
    }
    return best;
}

struct Case {            // the sequences of one scenario with their limits; edge[i] in {-1, 0, +1}: the limit of sequence i
    std::vector<Seq> seqs;                 // is set to (its smallest distance as a pattern) + edge[i]; -2: k as given
    std::vector<int32_t> k;
    std::vector<int> edge;
    std::vector<smx_hits_job> jobs;
    uint32_t add(const Seq &s, int kk, int e = -2) {
        seqs.push_back(s);
        k.push_back(kk);
        edge.push_back(e);
        return (uint32_t)seqs.size() - 1;
    }
};

struct Sim {
    std::mt19937_64 rng;
    std::map<std::string, long long> count;
    long long mismatches = 0, n_sample = 0;
    FILE *sample = nullptr;
    explicit Sim(uint64_t seed) : rng(seed) {}
    int uni(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }
    Seq rand_seq(int n, const Seq &alpha) {
        Seq s(n, 0);
        for (char &c : s) c = alpha[rng() % alpha.size()];
        return s;
    }
    Seq mutate(const Seq &s, double rate, const Seq &alpha) {
        Seq out;
        std::uniform_real_distribution<double> U(0.0, 1.0);
        for (char c : s) {
            const double r = U(rng);
            if (r < rate / 3) out.push_back(alpha[rng() % alpha.size()]);
            else if (r < 2 * rate / 3) { out.push_back(c); out.push_back(alpha[rng() % alpha.size()]); }
            else if (r >= rate) out.push_back(c);
        }
        if (out.empty()) out = s;
        return out;
    }
    int limit_for(const Seq &s) {          // the usual limit, now and then none
        return rng() % 9 == 0 ? -1 : (int)s.size() / 8;
    }
    void bad(const char *what, long long a, long long b, long long got, long long want) {
        if (++mismatches <= 20) printf("MISMATCH %s at (%lld, %lld): got %lld want %lld\n", what, a, b, got, want);
    }

    // Plan, run and check one case under one coverage bound, with K = 1, 3 and 16.
    void run_case(const char *name, Case &C, int cov) {
        const uint32_t n_seqs = (uint32_t)C.seqs.size();
        std::string bytes;
        std::vector<uint64_t> off{0};
        for (const Seq &s : C.seqs) { bytes += s; off.push_back(bytes.size()); }
        // the unlimited DP of every eligible pair under the pair rule, once; D keyed by job: D[j][(q - q0) * nt + t - t0]
        std::vector<std::vector<int>> D(C.jobs.size());
        auto pattern_is_query = [&](uint32_t q, uint32_t t) { return C.seqs[q].size() <= C.seqs[t].size(); };
        std::vector<int> dmin(n_seqs, INT32_MAX);  // per sequence: its smallest distance as a pattern
        for (size_t j = 0; j < C.jobs.size(); j++) {
            const smx_hits_job &J = C.jobs[j];
            D[j].assign((size_t)J.nq * J.nt, -2);  // -2: not eligible
            for (uint32_t q = J.q0; q < J.q0 + J.nq; q++)
                for (uint32_t t = J.t0; t < J.t0 + J.nt; t++) {
                    const bool pq = pattern_is_query(q, t);
                    const Seq &pat = pq ? C.seqs[q] : C.seqs[t], &txt = pq ? C.seqs[t] : C.seqs[q];
                    const long long lp = (long long)pat.size(), lt = (long long)txt.size();
                    if (lp * 1000 == (long long)cov * lt && cov > 0) count["cov_at_threshold"]++;
                    if (lp * 1000 < (long long)cov * lt && (lp + 1) * 1000 >= (long long)cov * lt) count["cov_one_short"]++;
                    if (lp * 1000 < (long long)cov * lt) { count["cov_excluded"]++; continue; }
                    const int d = dp_hw(pat, txt);
                    D[j][(size_t)(q - J.q0) * J.nt + (t - J.t0)] = d;
                    const uint32_t p = pq ? q : t;
                    dmin[p] = std::min(dmin[p], d);
                    if (lp == lt) {
                        count["equal_length_pairs"]++;
                        if (dp_hw(txt, pat) != d) count["tie_rule_pinned"]++;
                    }
                }
        }
        for (uint32_t i = 0; i < n_seqs; i++)
            if (C.edge[i] != -2 && dmin[i] != INT32_MAX) C.k[i] = std::max(0, dmin[i] + C.edge[i]);
        for (int K : {1, 3, 16}) {
            HitsPlan P;
            std::string why;
            if (hits_plan(bytes.data(), off.data(), n_seqs, C.jobs.data(), (uint32_t)C.jobs.size(), (uint32_t)K, (uint32_t)cov, &P,
                          &why) != SMX_OK) {
                printf("MISMATCH plan refused: %s\n", why.c_str());
                mismatches++;
                return;
            }
            // the reference: limited distances, and per query the K smallest keys by a full sort
            std::vector<int32_t> want_dist(P.n_dist, -1);
            std::vector<u64> want(P.n_rows * K, HITS_NONE);
            std::vector<std::vector<u64>> offers(P.n_rows);
            uint64_t eligible = 0;
            for (size_t j = 0; j < C.jobs.size(); j++) {
                const smx_hits_job &J = C.jobs[j];
                for (uint32_t q = J.q0; q < J.q0 + J.nq; q++) {
                    std::vector<u64> &mine = offers[P.jobs[j].row_off + (q - J.q0)];
                    for (uint32_t t = J.t0; t < J.t0 + J.nt; t++) {
                        const int d0 = D[j][(size_t)(q - J.q0) * J.nt + (t - J.t0)];
                        if (d0 == -2) continue;
                        eligible++;
                        const bool pq = pattern_is_query(q, t);
                        const uint32_t p = pq ? q : t;
                        const int lim = C.k[p];
                        const int d = (lim >= 0 && d0 > lim) ? -1 : d0;
                        want_dist[P.jobs[j].dist_off + (uint64_t)(q - J.q0) * J.nt + (t - J.t0)] = d;
                        if (K == 1) {
                            if (lim >= 0 && lim == d0 - 1) count["k_d_minus_1"]++;
                            if (lim == d0) count["k_d"]++;
                            if (lim == d0 + 1) count["k_d_plus_1"]++;
                            if (lim < 0) count["k_negative"]++;
                            count[pq ? "pairs_pattern_query" : "pairs_pattern_target"]++;
                            const Seq &pat = C.seqs[p], &txt = C.seqs[pq ? t : q];
                            if (pat.size() <= 300 && txt.size() <= 400 && rng() % 5 == 0) {
                                for (unsigned char c : pat) fprintf(sample, "%02x", c);
                                fprintf(sample, " ");
                                for (unsigned char c : txt) fprintf(sample, "%02x", c);
                                fprintf(sample, " %d %d\n", lim, d);
                                n_sample++;
                            }
                        }
                        if (d < 0) continue;
                        const u64 ppm = ((u64)d << 20) / (u64)C.seqs[p].size();
                        mine.push_back((ppm << 43) | ((u64)d << 24) | (u64)(t - J.t0));
                    }
                    std::sort(mine.begin(), mine.end());
                    for (size_t s = 0; s < mine.size() && s < (size_t)K; s++) want[(P.jobs[j].row_off + (q - J.q0)) * K + s] = mine[s];
                    if (mine.size() < (size_t)K) count["hits_fewer_than_K"]++;
                    else if (mine.size() == (size_t)K) count["hits_exactly_K"]++;
                    else if (mine.size() >= (size_t)4 * K) count["hits_many_more_than_K"]++;
                    for (size_t s = 1; s < mine.size() && s <= (size_t)K; s++)
                        if ((mine[s] >> 24) == (mine[s - 1] >> 24)) { count["ties_to_lower_index"]++; break; }
                }
            }
            if (P.n_pairs != eligible) bad("planned pairs", K, cov, (long long)P.n_pairs, (long long)eligible);
            if (K == 1) {                          // the windows the plan made, by side and size; the windows coverage emptied
                for (const HitsRec &R : P.recs) {
                    const std::string key = std::string(R.side ? "window_t_" : "window_q_") + std::to_string(R.n);
                    if (R.n == 1 || R.n == 127 || R.n == 128 || R.n == 129 || R.n == 257) count[key]++;
                }
                for (size_t j = 0; j < C.jobs.size(); j++) {
                    const smx_hits_job &J = C.jobs[j];
                    if (!J.nt) continue;
                    for (uint32_t q = J.q0; q < J.q0 + J.nq; q++) {
                        bool longer = false, any = false;
                        for (uint32_t t = J.t0; t < J.t0 + J.nt; t++) {
                            if (C.seqs[t].size() >= C.seqs[q].size()) longer = true;
                            if (C.seqs[t].size() >= C.seqs[q].size() && D[j][(size_t)(q - J.q0) * J.nt + (t - J.t0)] != -2) any = true;
                        }
                        if (longer && !any) count["windows_emptied"]++;
                    }
                }
            }
            const NearestHostSeqs S(bytes.data(), off.data(), n_seqs);
            std::vector<u64> scratch(P.scratch_words), keys(P.n_rows * K, HITS_NONE);
            for (u64 &w : scratch) w = rng();      // the kernel's scratch is never initialised either
            HitsHostCounts HC;
            hits_host_run(P, S, C.k.data(), K, keys.data(), nullptr, scratch.data(), &HC);   // the simulated lane order
            for (uint64_t i = 0; i < keys.size(); i++)
                if (keys[i] != want[i]) bad("key", K, (long long)i, (long long)keys[i], (long long)want[i]);
            if ((uint64_t)HC.pairs != eligible) bad("pair count", K, cov, HC.pairs, (long long)eligible);
            // hits_insert fed each query's offers in three shuffled orders: identical slots each time
            for (int round = 0; round < 3; round++)
                for (uint64_t r = 0; r < P.n_rows; r++) {
                    std::vector<u64> o = offers[r];
                    std::shuffle(o.begin(), o.end(), rng);
                    u64 slots[HITS_MAX_K];
                    for (int s = 0; s < K; s++) slots[s] = HITS_NONE;
                    for (u64 key : o) hits_insert(slots, K, key, HitsHostMin{nullptr});
                    for (int s = 0; s < K; s++)
                        if (slots[s] != want[r * K + s]) bad("shuffled insert", (long long)r, s, (long long)slots[s], (long long)want[r * K + s]);
                    count["shuffled_rows"]++;
                }
            std::vector<int32_t> dist(P.n_dist, -1);
            hits_host_run(P, S, C.k.data(), K, nullptr, dist.data(), scratch.data(), nullptr);
            for (uint64_t i = 0; i < P.n_dist; i++)
                if (dist[i] != want_dist[i]) bad("dist", K, (long long)i, dist[i], want_dist[i]);
            count["plans"]++;
            count["dist_checked"] += (long long)P.n_dist;
            count["pairs"] += HC.pairs;
            count["side_q_pairs"] += HC.side_pairs[0];
            count["side_t_pairs"] += HC.side_pairs[1];
            count["chunks"] += HC.chunks;
            count["builds"] += HC.builds;
            count["inserts"] += HC.inserts;
            count["atomics"] += HC.atomics;
            count["prechecked"] += HC.prechecked;
            static const char *cls[6] = {"class_0", "class_1", "class_2", "class_4", "class_8", "class_16"};
            for (int c = 0; c < 6; c++) count[cls[c]] += HC.class_pairs[c];
        }
        count[std::string("scenario_") + name]++;
    }

    // Patterns of every state class: per length a family of targets around a query -- with flanks (the query is the
    // pattern), trimmed (the target is), mutated copies, twins, strangers.  direction: 0 mixed, 1 queries all shorter
    // than the targets, 2 queries all longer.
    void classes(const char *name, const std::vector<int> &lens, int direction, int cov) {
        const Seq alpha = rng() % 2 ? Seq("ACGT") : Seq("ACGTN\x80");
        Case C;
        std::vector<Seq> roots;
        for (int m : lens) roots.push_back(rand_seq(m, alpha));
        const int longest = *std::max_element(lens.begin(), lens.end());
        for (const Seq &r : roots) {
            Seq q = r;
            if (direction == 2) q = rand_seq(longest + 5 - (int)r.size() / 2, alpha) + r + rand_seq(uni(1, 9), alpha);
            C.add(q, limit_for(q), rng() % 3 == 0 ? (int)(rng() % 3) - 1 : -2);
        }
        const uint32_t nq = (uint32_t)C.seqs.size();
        for (const Seq &r : roots) {
            const int m = (int)r.size();
            std::vector<Seq> fam;
            if (direction != 2) {                  // targets longer than the query: flanks of up to 60 bytes
                fam.push_back(rand_seq(uni(0, 60), alpha) + r + rand_seq(uni(1, 60), alpha));
                fam.push_back(rand_seq(uni(1, 60), alpha) + mutate(r, 0.04, alpha) + rand_seq(uni(0, 60), alpha));
                fam.push_back(rand_seq(longest + uni(1, 20), alpha));
            }
            if (direction != 1) {                  // targets shorter: trimmed, trimmed and mutated
                const int a = uni(0, m / 4), b = m - uni(0, m / 4);
                fam.push_back(r.substr(a, std::max(1, b - a)));
                fam.push_back(mutate(r.substr(a, std::max(1, b - a)), 0.04, alpha));
            }
            if (direction == 0) {
                fam.push_back(r);                  // equal length: the query is the pattern
                fam.push_back(mutate(r, 0.08, alpha));
                fam.push_back(rand_seq(m, alpha));
            }
            for (const Seq &t : fam) {
                Seq s = t;
                if (direction == 1 && (int)s.size() <= longest) s += rand_seq(longest + 1 - (int)s.size(), alpha);
                if (direction == 2 && (int)s.size() > longest) s = s.substr(0, longest);
                C.add(s, limit_for(s), rng() % 4 == 0 ? (int)(rng() % 3) - 1 : -2);
            }
        }
        C.add(C.seqs[nq], C.k[nq]);                // a twin of the first target, behind all others: ties to the lower index
        C.jobs.push_back(smx_hits_job{0, nq, nq, (uint32_t)C.seqs.size() - nq});
        run_case(name, C, cov);
    }

    // Windows of 1 / 127 / 128 / 129 / 257 texts on both sides, short sequences; one job per window, and a last job that
    // shares the targets of the first.
    void windows() {
        const Seq alpha = "ACGT";
        Case C;
        const int sizes[] = {1, 127, 128, 129, 257};
        std::vector<uint32_t> q_at, t_at;
        for (int n : sizes) {                      // side Q: one query of 40, n targets of 41..70 around it
            const Seq q = rand_seq(40, alpha);
            const uint32_t q0 = C.add(q, 5, (int)(rng() % 3) - 1);
            const uint32_t t0 = (uint32_t)C.seqs.size();
            for (int i = 0; i < n; i++) {
                const Seq core = i % 3 == 2 ? rand_seq(40, alpha) : mutate(q, 0.01 * uni(0, 20), alpha);
                const Seq t = rand_seq(uni(1, 15), alpha) + core + rand_seq(uni(1, 15), alpha);
                C.add(t.size() > 40 ? t : t + rand_seq(41 - (int)t.size(), alpha), 4);
            }
            C.jobs.push_back(smx_hits_job{q0, 1, t0, (uint32_t)n});
            q_at.push_back(q0);
            t_at.push_back(t0);
        }
        for (int n : sizes) {                      // side T: one target of 30, n queries of 31..60 that hold it, or not
            const Seq t = rand_seq(30, alpha);
            const uint32_t t0 = C.add(t, 4, (int)(rng() % 3) - 1);
            const uint32_t q0 = (uint32_t)C.seqs.size();
            for (int i = 0; i < n; i++) {
                const Seq core = i % 3 == 2 ? rand_seq(30, alpha) : mutate(t, 0.01 * uni(0, 20), alpha);
                const Seq q = rand_seq(uni(1, 15), alpha) + core + rand_seq(uni(1, 15), alpha);
                C.add(q.size() > 30 ? q : q + rand_seq(31 - (int)q.size(), alpha), 4);
            }
            C.jobs.push_back(smx_hits_job{q0, (uint32_t)n, t0, 1});
        }
        C.jobs.push_back(smx_hits_job{0, 0, t_at[1], 5});                 // no queries
        const uint32_t extra = C.add(rand_seq(40, alpha), -1);            // a query of its own over the 257 targets of job 4
        C.jobs.push_back(smx_hits_job{extra, 1, t_at[4], 257});           // jobs sharing targets
        C.add(rand_seq(12, alpha), 3);
        C.jobs.push_back(smx_hits_job{(uint32_t)C.seqs.size() - 1, 1, 0, 0});   // no targets: its row stays empty
        run_case("windows", C, 0);
    }

    // Coverage at the threshold and one byte short of it, on both sides; a window that coverage empties; an equal-length
    // pair whose two directions differ; many identical targets.
    void coverage() {
        const Seq alpha = "ACGT";
        Case C;
        const Seq q100 = rand_seq(100, alpha), q10 = rand_seq(10, alpha), q60 = rand_seq(60, alpha);
        // an equal-length pair with HW(q in t) != HW(t in q), found by search
        Seq ea, eb;
        for (int tries = 0; tries < 100000 && ea.empty(); tries++) {
            const Seq a = rand_seq(12, "AC"), b = rand_seq(12, "AC");
            if (dp_hw(a, b) != dp_hw(b, a)) { ea = a; eb = b; }
        }
        if (ea.empty()) { printf("MISMATCH no asymmetric pair found\n"); mismatches++; return; }
        C.add(q100, -1);
        C.add(q10, -1);
        C.add(q60, 12);
        C.add(ea, -1);
        const Seq q3 = rand_seq(45, alpha), q16 = rand_seq(46, alpha);    // exactly 3 and exactly 16 hits: limit 0, copies
        C.add(q3, 0);
        C.add(q16, 0);
        const uint32_t nq = (uint32_t)C.seqs.size();
        for (int i = 0; i < 3; i++) C.add(rand_seq(uni(1, 6), alpha) + q3 + rand_seq(uni(1, 6), alpha), 0);
        for (int i = 0; i < 16; i++) C.add(rand_seq(uni(1, 6), alpha) + q16 + rand_seq(uni(1, 6), alpha), 0);
        C.add(rand_seq(50, alpha) + q100 + rand_seq(50, alpha), -1);      // 200: exactly at 0.5 of q100
        C.add(rand_seq(50, alpha) + q100 + rand_seq(51, alpha), -1);      // 201: one byte short
        C.add(q100.substr(20, 50), -1);                                   // 50 in 100: at the threshold, the target is the pattern
        C.add(q100.substr(20, 49), -1);                                   // 49: one byte short
        C.add(eb, -1);                                                    // equal length with ea
        for (int i = 0; i < 40; i++) C.add(rand_seq(5, alpha) + q60 + rand_seq(5, alpha), 7);   // 40 twins ...
        const Seq twin = rand_seq(3, alpha) + mutate(q60, 0.05, alpha) + rand_seq(4, alpha);
        for (int i = 0; i < 40; i++) C.add(i % 2 ? twin : mutate(twin, 0.03, alpha), 7);        // ... and near twins
        C.jobs.push_back(smx_hits_job{0, nq, nq, (uint32_t)C.seqs.size() - nq});
        run_case("coverage", C, 500);
    }

    void refusals() {
        // from lengths alone: seqs = nullptr
        auto plan = [&](const std::vector<uint64_t> &off, const std::vector<smx_hits_job> &jobs, uint32_t K, uint32_t cov) {
            HitsPlan P;
            std::string why;
            return hits_plan(nullptr, off.data(), (uint32_t)off.size() - 1, jobs.data(), (uint32_t)jobs.size(), K, cov, &P, &why);
        };
        auto expect = [&](const char *what, int got, int want) {
            if (got != want) bad(what, 0, 0, got, want);
            else count["refusals_checked"]++;
        };
        const std::vector<uint64_t> off{0, 8, 16, 16, 20, 25};           // sequence 2 is empty
        expect("good", plan(off, {{0, 2, 3, 2}}, 5, 500), SMX_OK);
        expect("K 0", plan(off, {{0, 2, 3, 2}}, 0, 500), SMX_ERR_ARG);
        expect("K 17", plan(off, {{0, 2, 3, 2}}, 17, 500), SMX_ERR_ARG);
        expect("K 16", plan(off, {{0, 2, 3, 2}}, 16, 1000), SMX_OK);
        expect("cov 1001", plan(off, {{0, 2, 3, 2}}, 5, 1001), SMX_ERR_ARG);
        expect("empty query", plan(off, {{1, 2, 3, 2}}, 5, 500), SMX_ERR_ARG);
        expect("empty target", plan(off, {{0, 2, 2, 2}}, 5, 500), SMX_ERR_ARG);
        expect("empty target, no queries", plan(off, {{0, 0, 2, 2}}, 5, 500), SMX_ERR_ARG);
        expect("queries out of range", plan(off, {{4, 2, 0, 1}}, 5, 500), SMX_ERR_ARG);
        expect("targets out of range", plan(off, {{0, 1, 3, 3}}, 5, 500), SMX_ERR_ARG);
        expect("query ranges overlap", plan(off, {{0, 2, 3, 1}, {1, 1, 4, 1}}, 5, 500), SMX_ERR_ARG);
        expect("target ranges overlap", plan(off, {{0, 1, 3, 2}, {1, 1, 3, 2}}, 5, 500), SMX_OK);
        expect("nq = 0 and nt = 0", plan(off, {{0, 0, 3, 2}, {0, 2, 0, 0}}, 5, 500), SMX_OK);
        // a pattern of 2^19 bytes; one byte less is planned
        expect("pattern 2^19", plan({0, 1u << 19, (1u << 20) + 1}, {{0, 1, 1, 1}}, 5, 0), SMX_ERR_UNSUPPORTED);
        expect("pattern 2^19 - 1", plan({0, (1u << 19) - 1, 1u << 20}, {{0, 1, 1, 1}}, 5, 0), SMX_OK);
        expect("text 2^19, pattern short", plan({0, 100, 100 + (1u << 19)}, {{0, 1, 1, 1}}, 5, 0), SMX_OK);
        // 2^24 + 1 targets
        std::vector<uint64_t> big((size_t)(1u << 24) + 3);
        for (size_t i = 0; i < big.size(); i++) big[i] = i;
        expect("2^24 + 1 targets", plan(big, {{0, 1, 1, (1u << 24) + 1}}, 5, 500), SMX_ERR_UNSUPPORTED);
    }
};

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: hits_sim <seed>\n");
        return 2;
    }
    Sim S(strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 11);
    S.sample = fopen("oracle_sample.txt", "w");
    if (!S.sample) { perror("oracle_sample.txt"); return 2; }
    const std::vector<int> all{1, 63, 64, 65, 128, 129, 200, 300, 500, 700, 1024, 1025, 1100};
    S.classes("mixed", all, 0, 0);
    S.classes("shorter", {1, 64, 65, 129, 300, 700, 1025}, 1, 300);
    S.classes("longer", {1, 63, 128, 200, 500, 1024, 1100}, 2, 300);
    S.windows();
    S.coverage();
    S.refusals();
    fclose(S.sample);
    printf("oracle_sample %lld\n", S.n_sample);
    for (auto &kv : S.count) printf("%s %lld\n", kv.first.c_str(), kv.second);
    printf("%lld mismatches\n", S.mismatches);
    return 0;
}
