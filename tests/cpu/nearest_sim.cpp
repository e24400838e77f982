// CPU simulation of the crosstalk call (specimux_amd/csrc/smx_nearest.hip): the host plan (smx_nearest_plan.h) and the
// kernel as a host loop over the planned chunks (tests/cpu/nearest_host.h: pairs_pair and smx_nearest_core.h called as
// the kernel calls them), checked against a plain O(mn) DP with edlib's NW semantics reduced by a two-line reference.
// Built and run by tests/test_nearest_cpu.py (g++, no GPU).
//
//   nearest_sim <seed>      two scenarios (see main), each planned with several G; writes oracle_sample.txt in the cwd
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

#include "nearest_host.h"

using namespace smx;
typedef std::string Seq;

static int dp_unlimited(const Seq &q, const Seq &t) {   // NW: D[i][0] = i, D[0][j] = j
    const int m = (int)q.size(), n = (int)t.size();
    std::vector<int> col(m + 1);
    for (int i = 0; i <= m; i++) col[i] = i;
    for (int j = 0; j < n; j++) {
        int diag = col[0];
        col[0] = j + 1;
        const unsigned char c = (unsigned char)t[j];
        for (int i = 1; i <= m; i++) {
            const int up = col[i - 1] + 1, left = col[i] + 1, sub = diag + ((unsigned char)q[i - 1] == c ? 0 : 1);
            diag = col[i];
            col[i] = std::min(std::min(up, left), sub);
        }
    }
    return col[m];
}

static int limited(int d, int k) { return (k >= 0 && d > k) ? -1 : d; }

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
        return out;
    }
    void bad(const char *what, long long a, long long b, long long got, long long want) {
        if (++mismatches <= 20) printf("MISMATCH %s at (%lld, %lld): got %lld want %lld\n", what, a, b, got, want);
    }

    // One scenario: refs of the given lengths (plus planted duplicates), jobs of the given read counts, all jobs over all
    // refs but the last, which takes a sub-range.  ref_k0: the refs' limits are 0, so that a pair's limit is its read's.
    void scenario(const char *name, const std::vector<int> &ref_lens, const std::vector<int> &job_reads, bool ref_k0) {
        const Seq alpha = rng() % 2 ? Seq("ACGT") : Seq("ACGTN\x80");
        std::vector<Seq> seqs;
        std::vector<int32_t> k;
        std::vector<uint32_t> group;
        // refs: group = index, then duplicates of two refs: one in the original's group (a tie within `own` for its
        // reads, within `other` for everybody else's) and one in a group of its own (a tie across the two keys)
        for (int m : ref_lens) {
            seqs.push_back(rand_seq(m, alpha));
            group.push_back((uint32_t)seqs.size() - 1);
        }
        const uint32_t n_plain = (uint32_t)seqs.size();
        const uint32_t dup_a = n_plain / 2, dup_b = n_plain - 1;
        seqs.push_back(seqs[dup_a]); group.push_back(dup_a);
        seqs.push_back(seqs[dup_b]); group.push_back(1000);
        seqs.push_back(seqs[1]); group.push_back(1);              // and one of a short ref, same group
        const uint32_t nq = (uint32_t)seqs.size();
        for (uint32_t r = 0; r < nq; r++) k.push_back(ref_k0 ? 0 : (int)seqs[r].size() / 10);
        std::vector<smx_nearest_job> jobs;
        std::vector<int> edge;                                     // per read: -2 = not an edge read, else the offset from d
        edge.assign(nq, -2);
        for (size_t j = 0; j < job_reads.size(); j++) {
            const uint32_t t0 = (uint32_t)seqs.size();
            // the last job takes the refs [1, nq - 1): shared refs, another slice of every class list
            const bool sub = j + 1 == job_reads.size() && job_reads.size() > 1;
            for (int i = 0; i < job_reads[j]; i++) {
                const uint32_t src = (uint32_t)(rng() % nq);
                const int kind = (int)(rng() % 16);
                Seq s;
                int kk, e = -2;
                uint32_t g = group[src];
                if (kind == 0) { s = Seq(); kk = rng() % 2 ? -1 : (int)seqs[src].size(); count["empty_reads"]++; }
                else if (kind == 1) { s = rand_seq((int)seqs[src].size() + uni(0, 5), alpha); kk = (int)s.size() / 10; }   // unrelated
                else if (kind == 2) { s = seqs[src]; kk = 0; }                                    // identical: ties where src has a twin
                else if (kind <= 5) { s = mutate(seqs[src], 0.05, alpha); kk = 0; e = (kind - 3) - 1; }   // limit at d - 1, d, d + 1
                else if (kind == 6) { s = mutate(seqs[src], 0.05, alpha); kk = -1; }              // no limit
                else { s = mutate(seqs[src], 0.01 * uni(0, 12), alpha); kk = (int)s.size() / 10; }
                if (rng() % 4 == 0) g = group[rng() % nq];         // filed under another specimen
                if (rng() % 16 == 0) g = 77777;                    // or under one without a ref
                seqs.push_back(s);
                k.push_back(kk);
                group.push_back(g);
                edge.push_back(e);
            }
            jobs.push_back(sub ? smx_nearest_job{1, nq - 2, t0, (uint32_t)job_reads[j]} : smx_nearest_job{0, nq, t0, (uint32_t)job_reads[j]});
        }
        jobs.push_back(smx_nearest_job{0, nq, 0, 0});              // no reads
        seqs.push_back(seqs[0]); k.push_back(-1); group.push_back(0); edge.push_back(-2);
        jobs.push_back(smx_nearest_job{0, 0, (uint32_t)seqs.size() - 1, 1});   // no refs: its read keeps both keys all-ones
        // the unlimited DP of every pair of every job, once
        const uint32_t n_seqs = (uint32_t)seqs.size();
        std::vector<std::vector<int>> D(nq, std::vector<int>(n_seqs, -1));
        for (const smx_nearest_job &J : jobs)
            for (uint32_t q = J.q0; q < J.q0 + J.nq; q++)
                for (uint32_t t = J.t0; t < J.t0 + J.nt; t++) D[q][t] = dp_unlimited(seqs[q], seqs[t]);
        // edge reads: the limit at the nearest ref's distance - 1, + 0, + 1 (the refs' limits are 0 where ref_k0)
        for (size_t j = 0; j + 2 < jobs.size(); j++)
            for (uint32_t t = jobs[j].t0; t < jobs[j].t0 + jobs[j].nt; t++) {
                if (edge[t] == -2) continue;
                int dmin = INT32_MAX;
                for (uint32_t q = jobs[j].q0; q < jobs[j].q0 + jobs[j].nq; q++) dmin = std::min(dmin, D[q][t]);
                k[t] = std::max(0, dmin + edge[t]);
            }
        std::string bytes;
        std::vector<uint64_t> off{0};
        for (const Seq &s : seqs) { bytes += s; off.push_back(bytes.size()); }
        // the reference: limited distances, and per read the minimum key over its job's refs, own and other
        NearestPlan P;
        std::string why;
        if (nearest_plan(bytes.data(), off.data(), n_seqs, jobs.data(), (uint32_t)jobs.size(), &P, &why) != SMX_OK) {
            printf("MISMATCH plan refused: %s\n", why.c_str());
            mismatches++;
            return;
        }
        std::vector<int32_t> want_dist(P.n_dist);
        std::vector<u64> want_own(P.n_best, NEAREST_NONE), want_other(P.n_best, NEAREST_NONE);
        for (size_t j = 0; j < jobs.size(); j++) {
            const smx_nearest_job &J = jobs[j];
            for (uint32_t t = J.t0; t < J.t0 + J.nt; t++) {
                u64 &o = want_own[P.jobs[j].best_off + (t - J.t0)], &x = want_other[P.jobs[j].best_off + (t - J.t0)];
                for (uint32_t q = J.q0; q < J.q0 + J.nq; q++) {
                    const int lim = (k[q] < 0 || k[t] < 0) ? -1 : std::max(k[q], k[t]);
                    const int d = limited(D[q][t], lim);
                    want_dist[P.jobs[j].dist_off + (uint64_t)(q - J.q0) * J.nt + (t - J.t0)] = d;
                    if (lim >= 0 && lim == D[q][t] - 1) count["k_d_minus_1"]++;
                    if (lim == D[q][t]) count["k_d"]++;
                    if (lim == D[q][t] + 1) count["k_d_plus_1"]++;
                    if (d < 0) continue;
                    u64 &slot = group[q] == group[t] ? o : x;                       // the two-line reference
                    slot = std::min(slot, ((u64)d << 32) | q);
                    if (seqs[q].size() <= 300 && seqs[t].size() <= 400 && !seqs[t].empty() && rng() % 6 == 0) {
                        for (unsigned char c : seqs[q]) fprintf(sample, "%02x", c);
                        fprintf(sample, " ");
                        for (unsigned char c : seqs[t]) fprintf(sample, "%02x", c);
                        fprintf(sample, " %d %d\n", lim, d);
                        n_sample++;
                    }
                }
                if (o == NEAREST_NONE && x == NEAREST_NONE) count["reads_no_key"]++;
                if (o != NEAREST_NONE && x == NEAREST_NONE) count["reads_own_only"]++;
                if (o == NEAREST_NONE && x != NEAREST_NONE) count["reads_other_only"]++;
                if (o != NEAREST_NONE && x != NEAREST_NONE) {
                    count["reads_both"]++;
                    if ((o >> 32) == (x >> 32)) count["tie_across_keys"]++;
                }
                // ties within one key: at least two refs of one class at the winning distance
                for (int own_side = 0; own_side < 2; own_side++) {
                    const u64 key = own_side ? o : x;
                    if (key == NEAREST_NONE) continue;
                    int n_at = 0;
                    for (uint32_t q = J.q0; q < J.q0 + J.nq; q++) {
                        const int lim = (k[q] < 0 || k[t] < 0) ? -1 : std::max(k[q], k[t]);
                        if ((group[q] == group[t]) == (own_side == 1) && limited(D[q][t], lim) == (int)(key >> 32)) n_at++;
                    }
                    if (n_at > 1) count[own_side ? "tie_within_own" : "tie_within_other"]++;
                }
            }
        }
        const NearestHostSeqs S(bytes.data(), off.data(), n_seqs);
        // chunks at run length 1, then G = 1 (whole classes), G = that (runs of one) and two in between
        nearest_plan_runs(&P, UINT64_MAX);
        uint64_t at1 = 0;
        for (int c = 0; c < 6; c++) at1 += P.chunks[c];
        bool first = true;
        for (uint64_t G : {(uint64_t)1, UINT64_MAX, at1 * 2 / 3, at1 / 2, at1 / 3}) {
            nearest_plan_runs(&P, G);
            std::vector<u64> scratch(P.scratch_words), own(P.n_best, NEAREST_NONE), other(P.n_best, NEAREST_NONE);
            for (u64 &w : scratch) w = rng();      // the kernel's scratch is never initialised either
            NearestHostCounts C;
            nearest_host_run(P, S, k.data(), group.data(), own.data(), other.data(), nullptr, scratch.data(), &C);
            for (uint64_t i = 0; i < P.n_best; i++) {
                if (own[i] != want_own[i]) bad("own", (long long)G, (long long)i, (long long)own[i], (long long)want_own[i]);
                if (other[i] != want_other[i]) bad("other", (long long)G, (long long)i, (long long)other[i], (long long)want_other[i]);
            }
            if ((uint64_t)C.pairs != P.n_dist) bad("pair count", (long long)G, 0, C.pairs, (long long)P.n_dist);
            count["plans"]++;
            count["pairs"] += C.pairs;
            count["chunks"] += C.chunks;
            count["builds"] += C.builds;
            count["mins"] += C.mins;
            count["runs_of_one"] += C.runs_of_one;
            count["runs_of_class"] += C.runs_of_class;
            count["runs_between"] += C.runs_between;
            if (P.run_len == 1) count["plans_run_len_1"]++;
            else if (C.runs_between) count["plans_run_len_between"]++;
            else count["plans_run_len_class"]++;
            static const char *cls[6] = {"class_0", "class_1", "class_2", "class_4", "class_8", "class_16"};
            for (int c = 0; c < 6; c++) count[cls[c]] += C.class_pairs[c];
            if (first) {                           // distances mode, once
                std::vector<int32_t> dist(P.n_dist, -7);
                nearest_host_run(P, S, k.data(), group.data(), nullptr, nullptr, dist.data(), scratch.data(), nullptr);
                for (uint64_t i = 0; i < P.n_dist; i++)
                    if (dist[i] != want_dist[i]) bad("dist", 0, (long long)i, dist[i], want_dist[i]);
                count["dist_checked"] += (long long)P.n_dist;
                first = false;
            }
        }
        count[std::string("scenario_") + name]++;
    }
};

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: nearest_sim <seed>\n");
        return 2;
    }
    Sim S(strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 5);
    S.sample = fopen("oracle_sample.txt", "w");
    if (!S.sample) { perror("oracle_sample.txt"); return 2; }
    // every state class and the generic one, few reads; then short refs, every read count around the chunk size, two big
    // jobs sharing the refs
    S.scenario("classes", {1, 63, 64, 65, 128, 129, 1024, 1025, 1100, 200, 300, 500, 700}, {1, 127}, false);
    S.scenario("reads", {1, 63, 64, 65, 128, 129, 20, 40, 100}, {1, 127, 128, 129, 257}, true);
    fclose(S.sample);
    printf("oracle_sample %lld\n", S.n_sample);
    for (auto &kv : S.count) printf("%s %lld\n", kv.first.c_str(), kv.second);
    printf("%lld mismatches\n", S.mismatches);
    return 0;
}
