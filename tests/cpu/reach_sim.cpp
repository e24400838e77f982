// CPU simulation of the bimera call (specimux_amd/csrc/smx_reach.hip): the host plan (smx_reach_plan.h) and the kernel
// as a host loop over the planned chunks (tests/cpu/reach_host.h: smx_reach_core.h called as the kernel calls it),
// checked against the plain O(nm) DP of the definition -- D(i, j) anchored at both starts, reach(e) the largest i whose
// row minimum is <= e, the right side on the reversed strings -- reduced by a full sort.
// Built and run by tests/test_reach_cpu.py (g++, no GPU).
//
//   reach_sim <seed>     the scenarios of main, each with E = 0, 1, 5 and 15
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

#include "reach_host.h"

using namespace smx;
typedef std::string Seq;

// reach(q, r, e) for e = 0..E by the definition
static void dp_reach(const Seq &q, const Seq &r, int E, int *out) {
    const int n = (int)q.size(), m = (int)r.size();
    std::vector<int> row(m + 1), prev(m + 1);
    for (int e = 0; e <= E; e++) out[e] = 0;       // row 0: D(0, 0) = 0
    for (int j = 0; j <= m; j++) row[j] = j;
    for (int i = 1; i <= n; i++) {
        prev.swap(row);
        row[0] = i;
        int lo = row[0];
        for (int j = 1; j <= m; j++) {
            const int sub = prev[j - 1] + ((unsigned char)q[i - 1] == (unsigned char)r[j - 1] ? 0 : 1);
            row[j] = std::min(sub, std::min(prev[j], row[j - 1]) + 1);
            lo = std::min(lo, row[j]);
        }
        for (int e = 0; e <= E; e++)
            if (lo <= e) out[e] = i;
    }
}

struct Case {
    std::vector<Seq> seqs;
    std::vector<uint32_t> weight, need;
    std::vector<smx_reach_job> jobs;
    uint32_t add(const Seq &s, uint32_t w = 1, uint32_t nd = 0) {
        seqs.push_back(s);
        weight.push_back(w);
        need.push_back(nd);
        return (uint32_t)seqs.size() - 1;
    }
};

struct Sim {
    std::mt19937_64 rng;
    std::map<std::string, long long> count;
    long long mismatches = 0;
    explicit Sim(uint64_t seed) : rng(seed) {}
    int uni(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }
    Seq rand_seq(int n, const Seq &alpha = "ACGT") {
        Seq s(n, 0);
        for (char &c : s) c = alpha[rng() % alpha.size()];
        return s;
    }
    Seq edit(Seq s, int edits) {                   // `edits` random substitutions, insertions and deletions
        for (int x = 0; x < edits && !s.empty(); x++) {
            const size_t at = rng() % s.size();
            switch (rng() % 3) {
                case 0: s[at] = s[at] == 'A' ? 'C' : 'A'; break;
                case 1: s.insert(at, 1, "ACGT"[rng() % 4]); break;
                default: if (s.size() > 1) s.erase(at, 1); break;
            }
        }
        return s;
    }
    Seq flip(Seq s, size_t at) {                   // a substitution at one position, if the sequence has it
        if (at < s.size()) s[at] = s[at] == 'G' ? 'T' : 'G';
        return s;
    }
    void bad(const char *what, long long a, long long b, long long got, long long want) {
        if (++mismatches <= 20) printf("MISMATCH %s at (%lld, %lld): got %lld want %lld\n", what, a, b, got, want);
    }

    // Plan, run and check one case with E = 0, 1, 5 and 15.
    void run_case(const char *name, const Case &C) {
        const uint32_t n_seqs = (uint32_t)C.seqs.size();
        std::string bytes = "xyz";                 // the caller's array need not start at offset 0
        std::vector<uint64_t> off{bytes.size()};
        for (const Seq &s : C.seqs) {
            count[std::string("offset_mod8_") + std::to_string(bytes.size() % 8)]++;
            bytes += s;
            off.push_back(bytes.size());
        }
        const ReachHostSeqs S(bytes.data(), off.data(), n_seqs);
        if (S.rc != SMX_OK) { printf("MISMATCH sequences refused: %s\n", S.why.c_str()); mismatches++; return; }
        for (int E : {0, 1, 5, 15}) {
            ReachPlan P;
            std::string why;
            if (reach_plan(off.data(), n_seqs, C.jobs.data(), (uint32_t)C.jobs.size(), (uint32_t)E, &P, &why) != SMX_OK) {
                printf("MISMATCH plan refused: %s\n", why.c_str());
                mismatches++;
                return;
            }
            // the reference: the matrix by the DP, the keys by a full sort
            std::vector<uint32_t> want_values(P.n_values, REACH_NOT_ELIGIBLE);
            std::vector<u64> want(P.n_keys, HITS_NONE);
            std::vector<std::vector<u64>> offers(P.n_keys / REACH_SLOTS);
            long long eligible = 0;
            for (size_t j = 0; j < C.jobs.size(); j++) {
                const smx_reach_job &J = C.jobs[j];
                for (uint32_t q = J.q0; q < J.q0 + J.nq; q++) {
                    int n_elig = 0;
                    const Seq &qs = C.seqs[q], qr(qs.rbegin(), qs.rend());
                    for (uint32_t t = J.t0; t < J.t0 + J.nt; t++) {
                        if (E == 0) {
                            if (t == q) count["target_is_query"]++;
                            if (t != q && C.weight[t] == C.need[q]) count["weight_at_need"]++;
                            if (t != q && C.weight[t] + 1 == C.need[q]) count["weight_one_short"]++;
                        }
                        if (t == q || C.weight[t] < C.need[q]) continue;
                        n_elig++;
                        eligible++;
                        const Seq &ts = C.seqs[t], tr(ts.rbegin(), ts.rend());
                        int r[2][REACH_MAX_E + 1];
                        dp_reach(qs, ts, E, r[0]);
                        dp_reach(qr, tr, E, r[1]);
                        if (E == 15) classify(qs, ts, q, t, S, r[0]);
                        const uint64_t pair = P.jobs[j].mat_off + (uint64_t)(q - J.q0) * J.nt + (t - J.t0);
                        for (int side = 0; side < 2; side++)
                            for (int e = 0; e <= E; e++) {
                                want_values[reach_value_at(pair, side, e, E)] = (uint32_t)r[side][e];
                                offers[reach_slot_at(P.jobs[j].row_off + (q - J.q0), side, e, E) / REACH_SLOTS].push_back(
                                    ((u64)(0xffffffffu - (uint32_t)r[side][e]) << 32) | t);
                            }
                    }
                    if (E == 0) count[n_elig > 3 ? std::string("eligible_more") : "eligible_" + std::to_string(n_elig)]++;
                }
                if (E == 0) {
                    const uint64_t pairs = (uint64_t)J.nq * J.nt;
                    if (pairs <= 3 || (pairs >= 63 && pairs <= 65)) count["job_pairs_" + std::to_string(pairs)]++;
                    if (!J.nq) count["jobs_without_queries"]++;
                    if (!J.nt) count["jobs_without_targets"]++;
                }
            }
            for (size_t s = 0; s < offers.size(); s++) {
                std::vector<u64> o = offers[s];
                std::sort(o.begin(), o.end());
                for (size_t x = 0; x < o.size() && x < (size_t)REACH_SLOTS; x++) want[s * REACH_SLOTS + x] = o[x];
                if (o.size() >= 2 && (o[0] >> 32) == (o[1] >> 32)) count["ties_to_lower_index"]++;
            }
            std::vector<u64> keys(P.n_keys, HITS_NONE);
            ReachHostCounts HC;
            reach_host_run(P, S, n_seqs, C.weight.data(), C.need.data(), E, keys.data(), nullptr, &HC);
            for (uint64_t i = 0; i < keys.size(); i++)
                if (keys[i] != want[i]) bad("key", E, (long long)i, (long long)keys[i], (long long)want[i]);
            if (HC.items != 2 * eligible) bad("item count", E, 0, HC.items, 2 * eligible);
            std::vector<uint32_t> values(P.n_values, REACH_NOT_ELIGIBLE);
            reach_host_run(P, S, n_seqs, C.weight.data(), C.need.data(), E, nullptr, values.data(), nullptr);
            for (uint64_t i = 0; i < values.size(); i++)
                if (values[i] != want_values[i]) bad("value", E, (long long)i, values[i], want_values[i]);
            // hits_insert fed each slot pair's offers in three shuffled orders: identical slots each time
            for (int round = 0; round < 3; round++)
                for (size_t s = 0; s < offers.size(); s++) {
                    std::vector<u64> o = offers[s];
                    std::shuffle(o.begin(), o.end(), rng);
                    u64 slots[REACH_SLOTS] = {HITS_NONE, HITS_NONE};
                    for (u64 key : o) hits_insert(slots, REACH_SLOTS, key, ReachHostMin{nullptr});
                    for (int x = 0; x < REACH_SLOTS; x++)
                        if (slots[x] != want[s * REACH_SLOTS + x]) bad("shuffled insert", (long long)s, x, (long long)slots[x], (long long)want[s * REACH_SLOTS + x]);
                    count["shuffled_slots"]++;
                }
            count["plans"]++;
            count["values_checked"] += (long long)P.n_values;
            count["keys_checked"] += (long long)P.n_keys;
            count["chunks"] += HC.chunks;
            count["items"] += HC.items;
            count["not_eligible"] += HC.not_eligible;
            count["steps"] += HC.steps;
            count["slides"] += HC.slides;
            count["early_ends"] += HC.early;
            count["inserts"] += HC.inserts;
            count["atomics"] += HC.atomics;
            count["prechecked"] += HC.prechecked;
            count["side_left"] += HC.side_items[0];
            count["side_right"] += HC.side_items[1];
            for (int g = 0; g < 4; g++) count["group_" + std::to_string(g)] += HC.group_items[g];
            for (int x = 0; x < 8; x++) {
                count["slide_q_mod8_" + std::to_string(x)] += HC.slide_q_mod8[x];
                count["slide_r_mod8_" + std::to_string(x)] += HC.slide_r_mod8[x];
            }
        }
        count[std::string("scenario_") + name]++;
    }

    // what kind of pair this is (left side, E = 15), for the coverage counters
    void classify(const Seq &q, const Seq &t, uint32_t qi, uint32_t ti, const ReachHostSeqs &S, const int *r) {
        const size_t n = q.size(), m = t.size(), lo = std::min(n, m);
        size_t cp = 0;
        while (cp < lo && q[cp] == t[cp]) cp++;
        if (n > m) count["query_longer"]++;
        if (n < m) count["query_shorter"]++;
        if (q == t) count["identical_pairs"]++;
        if (cp == m && m < n) {                    // the target is a proper prefix: one more byte per further edit
            count["target_proper_prefix"]++;
            for (int e = 0; e <= REACH_MAX_E; e++)
                if (r[e] != (int)std::min(n, m + (size_t)e)) bad("proper prefix reach", qi, ti, r[e], (long long)std::min(n, m + (size_t)e));
        }
        if (cp == 0 && r[3] < (int)n && r[3] <= 12) count["unrelated_pairs"]++;
        if (cp == 7 || cp == 8 || cp == 9) count["first_mismatch_at_" + std::to_string(cp)]++;
        if (cp >= 15 && cp <= 17) count["first_mismatch_at_15_17"]++;
        // the match runs to the end of the shorter sequence and the bytes the kernel would read behind it are equal
        if (cp == lo && S.pad[S.doff[qi] + cp] == S.pad[S.doff[ti] + cp]) count["equal_beyond_the_end"]++;
        if (cp == lo && S.pad[S.doff[qi] + cp] == S.pad[S.doff[ti] + cp] && S.pad[S.doff[qi] + cp] != 0) count["equal_beyond_the_end_next_sequence"]++;
        if (n == 1 || m == 1) count["length_one"]++;
    }

    // Lengths 1, 7, 8, 9, 15, 16, 17, 63, 64, 65 on both sides: a family cut from the front of one root (related on the
    // left side) and one cut from the back of another (related on the right), every sequence a query and a target.
    void lengths() {
        const int lens[] = {1, 7, 8, 9, 15, 16, 17, 63, 64, 65};
        const Seq a = rand_seq(80), b = rand_seq(80);
        Case C;
        for (int L : lens) {
            const Seq fa = a.substr(0, L), fb = b.substr(80 - L);
            C.add(fa);                             // prefixes of one another: identical up to the shorter one's end
            C.add(fb);
            C.add(edit(fa, uni(1, 3)));
            C.add(edit(fb, uni(1, 3)));
            for (size_t at : {7, 8, 9, 15, 16, 17}) {          // the first mismatch at byte 7 / 8 / 9 of a slide, and of the second
                if ((size_t)L > at + 2) C.add(flip(fa, at));
                if ((size_t)L > at + 2) { Seq r = flip(Seq(fb.rbegin(), fb.rend()), at); C.add(Seq(r.rbegin(), r.rend())); }
            }
            C.add(rand_seq(L));                    // unrelated
            C.add(fa);                             // a twin: ties go to the lower index
        }
        const uint32_t n = (uint32_t)C.seqs.size();
        C.jobs.push_back(smx_reach_job{0, n, 0, n});
        run_case("lengths", C);
    }

    // A match to the end of the shorter sequence with equal bytes behind it: pairs of twins of 16 and 32 bytes (no
    // padding: the next sequence follows at once) followed by twins again, and shorter ones followed by zero padding.
    void padding() {
        const Seq root = rand_seq(96);
        Case C;
        for (int rep = 0; rep < 2; rep++) {
            C.add(root.substr(0, 16));
            C.add(root.substr(16, 32));
            C.add(root.substr(0, 32));
            C.add(root.substr(32, 16));
            C.add(root.substr(0, 48));
            C.add(root.substr(48, 48));
        }
        for (int L : {3, 8, 13, 24}) { C.add(root.substr(0, L)); C.add(root.substr(0, L) + "T"); }
        const uint32_t n = (uint32_t)C.seqs.size();
        C.jobs.push_back(smx_reach_job{0, n, 0, n});
        run_case("padding", C);
    }

    // Eligibility at weight = need and need - 1, t = q, identical targets, 0 / 1 / 2 / 3 / more eligible targets.
    void eligibility() {
        const Seq root = rand_seq(50);
        Case C;
        const uint32_t needs[] = {10, 9, 8, 7, 6, 5, 3, 0};
        for (uint32_t nd : needs) C.add(edit(root, uni(0, 4)), 1, nd);
        const uint32_t nq = (uint32_t)C.seqs.size();
        const Seq twin = edit(root, 2);
        C.add(edit(root, 1), 9);
        C.add(edit(root, 3), 7);
        C.add(twin, 5);
        C.add(twin, 5);
        C.add(edit(root, 2), 4);
        C.add(rand_seq(40), 3);
        C.jobs.push_back(smx_reach_job{0, nq, nq, (uint32_t)C.seqs.size() - nq});
        // the queries among themselves, every weight 1: need 0 takes all but itself
        C.add(edit(root, 1), 1, 0);
        C.jobs.push_back(smx_reach_job{(uint32_t)C.seqs.size() - 1, 1, 0, (uint32_t)C.seqs.size()});
        run_case("eligibility", C);
    }

    // Jobs of 1, 2, 3, 63, 64, 65 pairs, 129 targets (three chunks), jobs sharing targets, without queries, without targets.
    void shapes() {
        const Seq root = rand_seq(40);
        Case C;
        const int nts[] = {1, 2, 3, 63, 64, 65, 129};
        uint32_t shared_t0 = 0;
        for (int nt : nts) {
            const uint32_t q = C.add(edit(root, uni(0, 3)));
            const uint32_t t0 = (uint32_t)C.seqs.size();
            if (nt == 65) shared_t0 = t0;
            for (int i = 0; i < nt; i++) C.add(i % 5 == 4 ? rand_seq(uni(1, 45)) : edit(root.substr(0, uni(20, 40)), uni(0, 6)));
            C.jobs.push_back(smx_reach_job{q, 1, t0, (uint32_t)nt});
        }
        const uint32_t q2 = C.add(edit(root, 1));
        C.add(edit(root, 2));
        C.add(edit(root, 5));
        C.jobs.push_back(smx_reach_job{q2, 3, shared_t0, 65});            // three queries over the targets of the job of 65
        C.jobs.push_back(smx_reach_job{0, 0, shared_t0, 5});              // no queries
        const uint32_t lone = C.add(rand_seq(12));
        C.jobs.push_back(smx_reach_job{lone, 1, 0, 0});                   // no targets: its rows stay empty
        C.add("");                                                        // an empty sequence no job names
        run_case("shapes", C);
    }

    // Random pairs: lengths 0..40 would not pass the plan, so 1..70; truncated, extended, unrelated parents; other bytes.
    void random_pairs() {
        Case C;
        const Seq alpha = "ACGTN\x80";
        for (int x = 0; x < 60; x++) {
            const Seq q = rand_seq(uni(1, 70), alpha);
            const uint32_t qi = C.add(q);
            const uint32_t t0 = (uint32_t)C.seqs.size();
            C.add(edit(q, uni(0, 8)));
            C.add(edit(q.substr(0, uni(1, (int)q.size())), uni(0, 4)));
            C.add(edit(q, uni(0, 3)) + rand_seq(uni(1, 20), alpha));
            C.add(rand_seq(uni(1, 70), alpha));
            C.add(rand_seq(uni(0, 3), alpha) + q);                        // shifted: only edits at the start bring it back
            C.jobs.push_back(smx_reach_job{qi, 1, t0, 5});
        }
        run_case("random", C);
    }

    void refusals() {
        auto plan = [&](const std::vector<uint64_t> &off, const std::vector<smx_reach_job> &jobs, uint32_t E) {
            ReachPlan P;
            std::string why;
            return reach_plan(off.data(), (uint32_t)off.size() - 1, jobs.data(), (uint32_t)jobs.size(), E, &P, &why);
        };
        auto expect = [&](const char *what, int got, int want) {
            if (got != want) { printf("MISMATCH refusal %s\n", what); bad(what, 0, 0, got, want); }
            else count["refusals_checked"]++;
        };
        const std::vector<uint64_t> off{0, 8, 16, 16, 20, 25};           // sequence 2 is empty
        expect("good", plan(off, {{0, 2, 3, 2}}, 5), SMX_OK);
        expect("E 15", plan(off, {{0, 2, 3, 2}}, 15), SMX_OK);
        expect("E 16", plan(off, {{0, 2, 3, 2}}, 16), SMX_ERR_ARG);
        expect("empty query", plan(off, {{1, 2, 3, 2}}, 5), SMX_ERR_ARG);
        expect("empty target", plan(off, {{0, 2, 2, 2}}, 5), SMX_ERR_ARG);
        expect("empty target, no queries", plan(off, {{0, 0, 2, 2}}, 5), SMX_ERR_ARG);
        expect("queries out of range", plan(off, {{4, 2, 0, 1}}, 5), SMX_ERR_ARG);
        expect("targets out of range", plan(off, {{0, 1, 3, 3}}, 5), SMX_ERR_ARG);
        expect("query ranges overlap", plan(off, {{0, 2, 3, 1}, {1, 1, 4, 1}}, 5), SMX_ERR_ARG);
        expect("target ranges overlap", plan(off, {{0, 1, 3, 2}, {1, 1, 3, 2}}, 5), SMX_OK);
        expect("queries are targets", plan(off, {{0, 2, 0, 2}}, 5), SMX_OK);
        expect("nq = 0 and nt = 0", plan(off, {{0, 0, 3, 2}, {0, 2, 0, 0}}, 5), SMX_OK);
        expect("offsets fall", plan({0, 8, 4, 12}, {{0, 1, 2, 1}}, 5), SMX_ERR_ARG);
        expect("2^30 bytes", plan({0, 1u << 30, (1u << 30) + 5}, {{0, 1, 1, 1}}, 5), SMX_ERR_UNSUPPORTED);
        expect("2^30 - 1 bytes", plan({0, (1u << 30) - 1, (1u << 30) + 5}, {{0, 1, 1, 1}}, 5), SMX_OK);
    }
};

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: reach_sim <seed>\n");
        return 2;
    }
    Sim S(strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 19);
    S.lengths();
    S.padding();
    S.eligibility();
    S.shapes();
    S.random_pairs();
    S.refusals();
    for (auto &kv : S.count) printf("%s %lld\n", kv.first.c_str(), kv.second);
    printf("%lld mismatches\n", S.mismatches);
    return 0;
}
