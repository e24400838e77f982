// CPU simulation of the error-profile kernel (specimux_amd/csrc/smx_profile.hip): its body as a host loop
// (tests/cpu/profile_host.h) over the plans of smx_cons_plan.h and the host/device core smx_profile_core.h, checked against
// plain loops over the rows that apply the rules of DESIGN.md §21 as they are written there: a walk over the row with a
// running read position, and the draft's runs found by a scan of their own.  Built and run by tests/test_profile_cpu.py
// (g++, no GPU) and, under the sanitizers, by tests/asan/profile_driver.cpp.
//
//   profile_sim exhaustive       every row over drafts of 1..4 columns whose columns are a match, a sub, a deletion or another
//                                byte with an insertion of 0, 1, 2 or 5 bases before each and behind the last, for drafts
//                                with runs of every length up to 4 and with an `N`
//   profile_sim random <seed>    calls of 1..7 jobs of 0..70 members around drafts of 1..300 nt with homopolymer runs and
//                                `N` bytes, members above their limit, indels, a clipped insertion, quality bytes 0..255;
//                                the rows come from the full-matrix reference walk of tests/cpu/cons_sim.cpp
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

#include "profile_host.h"

using namespace smx;
typedef std::string Seq;

static long long mismatches = 0;
static std::map<std::string, long long> count;

static void bad(const char *what, long long a = 0, long long b = 0, long long c = 0) {
    if (++mismatches <= 20) printf("MISMATCH %s %lld %lld %lld\n", what, a, b, c);
}

static unsigned code_of(unsigned char c) {
    switch (c) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
        default: return 4;
    }
}

// cons_sim.cpp's reference: NW over the full matrix (D[i][0] = i, D[0][j] = j), then the walk from (m, n)
static int dp_row(const Seq &q, const Seq &t, uint32_t *row) {
    const int m = (int)q.size(), n = (int)t.size();
    std::vector<int> D((size_t)(m + 1) * (n + 1));
    auto at = [&](int i, int j) -> int & { return D[(size_t)i * (n + 1) + j]; };
    for (int i = 0; i <= m; i++) at(i, 0) = i;
    for (int j = 0; j <= n; j++) at(0, j) = j;
    for (int i = 1; i <= m; i++)
        for (int j = 1; j <= n; j++)
            at(i, j) = std::min(std::min(at(i - 1, j) + 1, at(i, j - 1) + 1), at(i - 1, j - 1) + (q[i - 1] != t[j - 1]));
    std::vector<unsigned> sym(m + 1, 7), ilen(m + 1, 0);
    std::vector<std::vector<unsigned>> ins(m + 1);
    int i = m, j = n;
    while (i > 0 || j > 0) {
        if (i > 0 && j > 0 && at(i - 1, j - 1) + (q[i - 1] != t[j - 1]) == at(i, j)) {
            sym[i - 1] = code_of((unsigned char)t[j - 1]);
            i--, j--;
        } else if (i > 0 && at(i - 1, j) + 1 == at(i, j)) {
            sym[i - 1] = 5;
            i--;
        } else {
            ins[i].push_back(code_of((unsigned char)t[j - 1]));
            ilen[i]++;
            j--;
        }
    }
    for (int p = 0; p <= m; p++) {
        std::reverse(ins[p].begin(), ins[p].end());
        uint32_t w = sym[p] | (std::min(ilen[p], 255u) << 3);
        for (size_t s = 0; s < ins[p].size() && s < SMX_CONS_MAX_INS; s++) w |= ins[p][s] << (11 + 3 * s);
        row[p] = w;
    }
    return at(m, n);
}

// ---- the rules again, one member: a walk with a running read position, then the runs
struct Ref {
    uint32_t words[SMX_PROFILE_MEMBER_WORDS] = {0};
    uint32_t t[SMX_PROFILE_JOB_WORDS] = {0};
    uint64_t consumed = 0;
};

static unsigned bin_of(unsigned char b) { return b < 33 ? 0u : std::min<unsigned>(b - 33u, 63u); }

static Ref ref_member(const Seq &draft, const uint32_t *row, const unsigned char *qual, size_t qlen) {
    Ref R;
    const size_t m = draft.size();
    bool clipped = false;
    for (size_t p = 0; p <= m; p++) clipped = clipped || ((row[p] >> 3) & 255) == 255;
    uint64_t rp = 0;
    uint32_t q[192] = {0};
    for (size_t p = 0; p <= m; p++) {
        const unsigned sym = row[p] & 7, L = (row[p] >> 3) & 255;
        if (L) {
            R.words[4]++;
            R.words[5] += L;
            for (unsigned i = 0; i < std::min(L, 4u); i++) R.t[212 + ((row[p] >> (11 + 3 * i)) & 7)]++;
            R.t[217] += L - std::min(L, 4u);
            for (unsigned i = 0; i < L; i++, rp++)
                if (!clipped) {
                    if (rp >= qlen) { bad("ref read position", (long long)rp, (long long)qlen); return R; }
                    q[bin_of(qual[rp]) * 3 + 2]++;
                }
        }
        if (p == m) break;
        const unsigned dc = code_of((unsigned char)draft[p]);
        int kind;                                              // q's column; -1: no read base
        if (sym == 5) { R.words[2]++; kind = -1; }
        else if (sym <= 3 && dc <= 3 && sym == dc) { R.words[0]++; kind = 0; }
        else if (sym <= 3 && dc <= 3) { R.words[1]++; kind = 1; }
        else { R.words[3]++; kind = 1; }
        if (dc <= 3 && (sym <= 3 || sym == 5)) R.t[192 + dc * 5 + (sym == 5 ? 4 : sym)]++;
        if (kind >= 0) {
            if (!clipped) {
                if (rp >= qlen) { bad("ref read position", (long long)rp, (long long)qlen); return R; }
                q[bin_of(qual[rp]) * 3 + kind]++;
            }
            rp++;
        }
    }
    R.words[6] = clipped;
    R.consumed = rp;
    if (!clipped) {
        memcpy(R.t, q, sizeof q);
        if (rp != qlen) bad("consumed != read length", (long long)rp, (long long)qlen);
    }
    for (size_t s = 0; s < m;) {
        const unsigned b = code_of((unsigned char)draft[s]);
        size_t e = s;
        while (e < m && code_of((unsigned char)draft[e]) == b) e++;
        if (b <= 3) {
            const size_t r = e - s;
            long long obs = 0;
            for (size_t p = s; p < e; p++) obs += (row[p] & 7) == b;
            for (size_t p = s; p <= e; p++) {
                const unsigned L = (row[p] >> 3) & 255;
                for (unsigned i = 0; i < std::min(L, 4u); i++) obs += ((row[p] >> (11 + 3 * i)) & 7) == b;
            }
            const long long delta = std::max(-3ll, std::min(3ll, obs - (long long)r));
            R.t[218 + (std::min<size_t>(r, 8) - 1) * 7 + (size_t)(delta + 3)]++;
            count["runs_seen"]++;
            if (r >= 8) count["runs_class_8"]++;
            if (obs - (long long)r <= -3 || obs - (long long)r >= 3) count["runs_at_clamp"]++;
            if (s / 64 != (e - 1) / 64) count["runs_across_batches"]++;
        }
        s = e;
    }
    return R;
}

struct Reads {
    std::string bytes, quals;
    std::vector<uint64_t> off{0};
    std::vector<int32_t> k;
    std::vector<Seq> seq;
    uint32_t add(const Seq &s, int kk, std::mt19937_64 &rng, int qmode) {
        bytes += s;
        for (size_t i = 0; i < s.size(); i++) {
            const unsigned edges[] = {0, 32, 33, 34, 95, 96, 97, 126, 255};
            quals.push_back((char)(qmode == 0 ? 33 + rng() % 50 : qmode == 1 ? rng() % 256 : edges[rng() % 9]));
        }
        off.push_back(bytes.size());
        k.push_back(kk);
        seq.push_back(s);
        return (uint32_t)k.size() - 1;
    }
};

static const uint32_t SENTINEL32 = 0xDEADBEEFu;

// One call the way the kernel sees it, over rows given or (rows == nullptr) made by dp_row, against ref_member
static void check_call(const Reads &R, const std::vector<smx_cons_job> &jobs, const std::vector<uint32_t> *given, std::mt19937_64 &rng) {
    ConsPlan P;
    std::string why;
    const uint32_t n_jobs = (uint32_t)jobs.size();
    if (cons_plan(R.bytes.data(), R.off.data(), (uint32_t)R.k.size(), R.k.data(), jobs.data(), n_jobs, CONS_HIST_BYTES, &P, &why) != SMX_OK ||
        cons_plan_profile(true, true, true, &P, &why) != SMX_OK) {
        bad(why.c_str());
        return;
    }
    if (P.member_words != P.n_dist * SMX_PROFILE_MEMBER_WORDS || P.table_words != (uint64_t)n_jobs * SMX_PROFILE_JOB_WORDS)
        bad("plan sizes", (long long)P.member_words, (long long)P.table_words);
    std::vector<uint32_t> rows(P.rows_words);
    std::vector<int32_t> dist(P.n_dist);
    if (given) {
        rows = *given;
        std::fill(dist.begin(), dist.end(), 0);
    } else
        for (uint32_t j = 0; j < n_jobs; j++) {
            const ConsJobDev &J = P.jobs[j];
            const int m = P.len[J.draft];
            for (uint32_t i = 0; i < J.n; i++) {
                const uint32_t r = J.r0 + i;
                uint32_t *row = rows.data() + J.rows_off + (size_t)i * (m + 1);
                const int d = dp_row(R.seq[J.draft], R.seq[r], row);
                const int k = (R.k[J.draft] < 0 || R.k[r] < 0) ? -1 : std::max(R.k[J.draft], R.k[r]);
                dist[J.dist_off + i] = (k >= 0 && d > k) ? -1 : d;
                if (dist[J.dist_off + i] < 0) {                // the kernel leaves no row for such a member: junk
                    for (int p = 0; p <= m; p++) row[p] = (uint32_t)rng();
                    count["members_above_limit"]++;
                }
            }
        }
    std::vector<uint32_t> per_member(P.member_words, SENTINEL32), tables(P.table_words, 0u);
    profile_host(P, R.bytes.data(), R.off.data(), rows.data(), dist.data(), (const unsigned char *)R.quals.data(), per_member.data(),
                 tables.data());
    for (uint32_t j = 0; j < n_jobs; j++) {
        const ConsJobDev &J = P.jobs[j];
        const Seq &draft = R.seq[J.draft];
        const size_t m = draft.size();
        uint32_t want[SMX_PROFILE_JOB_WORDS] = {0};
        count["jobs"]++;
        if (J.n == 0) count["jobs_without_members"]++;
        for (uint32_t i = 0; i < J.n; i++) {
            const uint32_t *got = per_member.data() + (J.dist_off + i) * SMX_PROFILE_MEMBER_WORDS;
            Ref ref;
            if (dist[J.dist_off + i] >= 0) {
                const uint32_t r = J.r0 + i;
                ref = ref_member(draft, rows.data() + J.rows_off + (size_t)i * (m + 1), (const unsigned char *)R.quals.data() + R.off[r],
                                 R.off[r + 1] - R.off[r]);
                count["members"]++;
                count["columns"] += (long long)m;
                count["subs"] += ref.words[1], count["dels"] += ref.words[2], count["others"] += ref.words[3];
                count["ins_events"] += ref.words[4];
                if (ref.words[6]) count["members_clipped"]++;
                if (ref.words[0] + ref.words[1] + ref.words[3] == 0) count["members_empty"]++;
            }
            if (memcmp(got, ref.words, sizeof ref.words)) bad("member words", j, i, got[0]);
            for (unsigned x = 0; x < SMX_PROFILE_JOB_WORDS; x++) want[x] += ref.t[x];
        }
        for (unsigned x = 0; x < SMX_PROFILE_JOB_WORDS; x++)
            if (tables[(size_t)j * SMX_PROFILE_JOB_WORDS + x] != want[x]) bad("table word", j, x, want[x]);
        for (unsigned x = 0; x < 192; x++) count["q_bases"] += want[x];
        count["q_bin_0"] += want[0] + want[1] + want[2];
        count["q_bin_63"] += want[189] + want[190] + want[191];
        count["ins_beyond_kept"] += want[217];
    }
}

// the row words of one member over `draft`: kinds[p] in {0 match, 1 sub, 2 del, 3 other}, lens[p] for p <= m; the inserted
// codes before p count up from the draft's code there, so that the first equals the run's base and the next does not
static void make_row(const Seq &draft, const unsigned *kinds, const unsigned *lens, uint32_t *row, size_t *consumed) {
    const size_t m = draft.size();
    *consumed = 0;
    for (size_t p = 0; p <= m; p++) {
        const unsigned dc = code_of((unsigned char)draft[p < m ? p : m - 1]);
        unsigned sym = 7;
        if (p < m) sym = kinds[p] == 0 ? (dc <= 3 ? dc : 0) : kinds[p] == 1 ? (dc + 1) % 4 : kinds[p] == 2 ? 5 : 4;
        uint32_t w = sym | (lens[p] << 3);
        for (unsigned i = 0; i < std::min(lens[p], 4u); i++) w |= ((dc + i) % 5) << (11 + 3 * i);
        row[p] = w;
        *consumed += lens[p] + (p < m && sym <= 4);
    }
}

static void run_exhaustive() {
    std::mt19937_64 rng(7);
    const unsigned lens_of[4] = {0, 1, 2, 5};
    const std::vector<Seq> drafts = {"A", "N", "AA", "AC", "NA", "AAA", "AAC", "ACA", "CNC", "AAAA", "AACC", "ACGT", "ANAA", "CAAT"};
    for (const Seq &draft : drafts) {
        const size_t m = draft.size();
        size_t n_rows = 4;
        for (size_t p = 0; p < m; p++) n_rows *= 16;
        Reads R;
        std::vector<uint32_t> rows(n_rows * (m + 1));
        for (size_t x = 0; x < n_rows; x++) {
            unsigned kinds[4], lens[5];
            size_t v = x;
            for (size_t p = 0; p < m; p++, v /= 16) kinds[p] = v % 4, lens[p] = lens_of[(v / 4) % 4];
            lens[m] = lens_of[v % 4];
            size_t consumed;
            make_row(draft, kinds, lens, rows.data() + x * (m + 1), &consumed);
            R.add(Seq(consumed, 'A'), -1, rng, 2);
            count["rows"]++;
        }
        const uint32_t d = R.add(draft, -1, rng, 0);
        check_call(R, {smx_cons_job{d, 0, (uint32_t)n_rows}}, &rows, rng);
    }
}

static void run_random(uint64_t seed) {
    std::mt19937_64 rng(seed * 0x9E3779B97F4A7C15ull + 77);
    auto uni = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    auto rand_seq = [&](int n) {                                 // with runs: a base is repeated 1..10 times
        Seq s;
        while ((int)s.size() < n) s.append((size_t)(rng() % 3 ? 1 : uni(2, 10)), "ACGT"[rng() % 4]);
        s.resize(n);
        return s;
    };
    auto mutate = [&](const Seq &s, int per_mille) {
        Seq out;
        for (char c : s) {
            const int r = (int)(rng() % 1000);
            if (r < per_mille) out.push_back("ACGTN"[rng() % 5]);
            else if (r < 2 * per_mille) { out.push_back(c); out.append((size_t)uni(1, 6), rng() % 2 ? c : "ACGT"[rng() % 4]); }
            else if (r >= 3 * per_mille) out.push_back(c);
        }
        return out;
    };
    const std::vector<int> sizes = {1, 2, 0, 63, 64, 65, 5, 17, 70, 0, 16};
    const std::vector<int> lens = {1, 2, 5, 63, 64, 65, 127, 128, 129, 300};
    int made = 0;
    for (int call = 0; call < 12; call++) {
        Reads R;
        std::vector<smx_cons_job> jobs;
        const int n_jobs = call == 0 ? 1 : uni(2, 7);
        for (int g = 0; g < n_jobs; g++, made++) {
            const int m = made < (int)lens.size() ? lens[made] : uni(1, 200);
            const int n = sizes[made % sizes.size()];
            Seq draft = rand_seq(m);
            if (made % 4 == 1) draft[uni(0, m - 1)] = 'N';
            if (m >= 70) draft.replace(60, 7, 7, 'G');                         // a run over the first batch edge
            const uint32_t r0 = (uint32_t)R.k.size();
            for (int i = 0; i < n; i++) {
                const int kind = (int)(rng() % 8);
                Seq s = mutate(draft, kind < 2 ? 0 : 40);
                int k = kind == 7 ? -1 : m / 3 + 8;
                if (kind == 6) { s = rand_seq(m + 30); k = m / 10; }           // above its limit
                if (kind == 5 && m >= 2) { s.insert((size_t)uni(0, (int)s.size()), (size_t)uni(255, 270), 'T'); k = -1; }   // clipped
                if (kind == 4) { s.erase(0, 1); if (!s.empty()) s.pop_back(); }  // deletions at both ends
                R.add(s, k, rng, i % 3);
            }
            const uint32_t d = made % 2 ? R.add(draft, m / 3 + 8, rng, 0) : (n ? r0 + (uint32_t)uni(0, n - 1) : R.add(draft, -1, rng, 0));
            jobs.push_back(smx_cons_job{d, r0, (uint32_t)n});
        }
        // a job whose draft is one of its members must not be an empty read
        for (smx_cons_job &J : jobs)
            if (R.seq[J.draft].empty()) J.draft = R.add("ACGT", -1, rng, 0);
        check_call(R, jobs, nullptr, rng);
        count["calls"]++;
    }
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "exhaustive")) {
        run_exhaustive();
    } else if (argc >= 3 && !strcmp(argv[1], "random")) {
        run_random(strtoull(argv[2], nullptr, 10));
    } else {
        fprintf(stderr, "usage: profile_sim exhaustive | random <seed>\n");
        return 2;
    }
    for (auto &kv : count) printf("%s %lld\n", kv.first.c_str(), kv.second);
    printf("%lld mismatches\n", mismatches);
    return 0;
}
