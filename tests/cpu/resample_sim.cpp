// CPU simulation of the resampling kernel (specimux_amd/csrc/smx_resample.hip): its body as a host loop
// (tests/cpu/resample_host.h) over the plans of smx_cons_plan.h and the host/device core smx_resample_core.h, checked
// against plain loops that build every replicate's 26-word vote table with cons_vote_word and apply the rule of DESIGN.md
// §20 as it is written there.  The rows come from the full-matrix reference walk of tests/cpu/cons_sim.cpp (dp_row below
// is that function), not from the banded code.  Built and run by tests/test_resample_cpu.py (g++, no GPU).
//
//   resample_sim exhaustive       resample_keeps over every (a[4], del, ins) a replicate of n_b <= 6 voters can have, every
//                                 draft code 0..4 and both p == m values, against one column of the call rule written out
//   resample_sim random <seed>    calls of 1..7 jobs of 0..200 members around drafts of 1..300 nt, 1..16 levels, with
//                                 members above their limit, `N` bytes, indels, and masks of every shape
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

#include "resample_host.h"

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

// ---- the rule again.  One column of consensus.call_consensus, written out: what the call emits before and at position
// p of a draft whose byte there has the code dc, from the position's 26 vote words of n voters; kept when that is the
// draft's byte and nothing else.  `draft_byte` stands for the byte: 'A'..'T' for dc < 4, 'N' otherwise.
static bool ref_keeps_by_call(const uint32_t *v, uint32_t n, unsigned dc, bool last) {
    const char draft_byte = dc < 4 ? "ACGT"[dc] : 'N';
    std::string out;
    int inserted = 0;
    for (unsigned s = 0; s < SMX_CONS_MAX_INS; s++) {
        const uint32_t *slot = v + 6 + 5 * s;
        if (2ull * (slot[0] + slot[1] + slot[2] + slot[3] + slot[4]) <= n) break;
        unsigned best = 0;
        for (unsigned c = 1; c < 4; c++)
            if (slot[c] > slot[best]) best = c;
        out.push_back("ACGT"[best]);
        inserted++;
    }
    if (!last && !(2ull * v[5] > n)) {
        const uint32_t top = std::max(std::max(v[0], v[1]), std::max(v[2], v[3]));
        if (top == 0) out.push_back(draft_byte);
        else {
            std::vector<unsigned> tied;
            for (unsigned c = 0; c < 4; c++)
                if (v[c] == top) tied.push_back(c);
            const bool mine = dc < 4 && std::find(tied.begin(), tied.end(), dc) != tied.end();
            out.push_back(mine ? draft_byte : "ACGT"[tied[0]]);
        }
    }
    // not a comparison of strings: an inserted base followed by a dropped one can spell the draft's byte again (a table
    // no alignment produces, but the exhaustive run builds it), and that is two edits, not a column kept
    return inserted == 0 && (last || out == std::string(1, draft_byte));
}

// the rule as DESIGN.md §20 writes it, over the 26 vote words
static bool ref_keeps_as_written(const uint32_t *v, uint32_t n_b, unsigned dc, bool last) {
    const uint64_t ins = (uint64_t)v[6] + v[7] + v[8] + v[9] + v[10], del = v[5];
    const uint32_t top = std::max(std::max(v[0], v[1]), std::max(v[2], v[3]));
    return !(2 * ins > n_b) && (last || (!(2 * del > n_b) && (top == 0 || (dc < 4 && v[dc] == top))));
}

static void run_exhaustive() {
    for (uint32_t n_b = 0; n_b <= 6; n_b++)
        for (uint32_t a0 = 0; a0 <= n_b; a0++)
            for (uint32_t a1 = 0; a0 + a1 <= n_b; a1++)
                for (uint32_t a2 = 0; a0 + a1 + a2 <= n_b; a2++)
                    for (uint32_t a3 = 0; a0 + a1 + a2 + a3 <= n_b; a3++)
                        for (uint32_t del = 0; a0 + a1 + a2 + a3 + del <= n_b; del++)
                            for (uint32_t ins = 0; ins <= n_b; ins++)
                                for (unsigned dc = 0; dc <= 4; dc++)
                                    for (int last = 0; last < 2; last++) {
                                        const uint32_t a[4] = {a0, a1, a2, a3};
                                        uint32_t v[SMX_CONS_VOTE_WORDS] = {0};
                                        memcpy(v, a, sizeof a);
                                        v[4] = n_b - (a0 + a1 + a2 + a3 + del);          // the voters with another byte
                                        v[5] = del;
                                        v[6 + dc] = ins / 2;                               // slot 0 over two of its codes
                                        v[6 + (dc + 2) % 5] += ins - ins / 2;
                                        const bool got = resample_keeps(a, del, ins, n_b, dc, last != 0);
                                        if (got != ref_keeps_by_call(v, n_b, dc, last != 0)) bad("keeps vs call", n_b, dc, last);
                                        if (got != ref_keeps_as_written(v, n_b, dc, last != 0)) bad("keeps vs rule", n_b, dc, last);
                                        count["cases"]++;
                                        count[got ? "kept" : "not_kept"]++;
                                        if (last) { count["last_cases"]++; if (2 * ins == n_b && n_b) count["last_half_insertions"]++; continue; }
                                        const uint32_t top = std::max(std::max(a0, a1), std::max(a2, a3));
                                        int tied = 0;
                                        for (unsigned c = 0; c < 4; c++) tied += a[c] == top;
                                        if (top > 0 && tied > 1 && dc < 4 && a[dc] == top) count["draft_wins_tie"]++;
                                        if (top > 0 && tied > 1 && (dc == 4 || a[dc] != top)) count["tie_without_draft"]++;
                                        if (n_b && 2 * del == n_b) count["half_deletions"]++;
                                        if (n_b && 2 * ins == n_b) count["half_insertions"]++;
                                        if (top == 0) count["top_zero"]++;
                                        if (dc == 4) count["other_draft"]++;
                                        if (dc == 4 && top == 0 && got) count["other_draft_kept"]++;
                                    }
    // counts that need 33 bits when doubled
    const uint32_t big[4] = {0x90000000u, 0, 0, 0};
    if (resample_keeps(big, 0, 0x80000001u, 0xffffffffu, 0, false) || !resample_keeps(big, 0, 0x7fffffffu, 0xffffffffu, 0, false) ||
        resample_keeps(big, 0x80000000u, 0, 0xffffffffu, 0, false))
        bad("keeps64");
}

struct Reads {
    std::string bytes;
    std::vector<uint64_t> off{0};
    std::vector<int32_t> k;
    std::vector<Seq> seq;
    uint32_t add(const Seq &s, int kk) {
        bytes += s;
        off.push_back(bytes.size());
        k.push_back(kk);
        seq.push_back(s);
        return (uint32_t)k.size() - 1;
    }
};

static const uint64_t SENTINEL64 = 0xDEADBEEFDEADBEEFull;
static const uint32_t SENTINEL32 = 0xDEADBEEFu;

// One call the way the kernel sees it, against plain loops over the members
static void check_call(const Reads &R, const std::vector<smx_cons_job> &jobs, uint32_t n_levels, std::mt19937_64 &rng) {
    ConsPlan P;
    std::string why;
    const uint32_t n_jobs = (uint32_t)jobs.size();
    if (cons_plan(R.bytes.data(), R.off.data(), (uint32_t)R.k.size(), R.k.data(), jobs.data(), n_jobs, CONS_HIST_BYTES, &P, &why) != SMX_OK ||
        cons_plan_resample(true, n_levels, &P, &why) != SMX_OK) {
        bad(why.c_str());
        return;
    }
    const uint64_t total = P.member_off.back();
    if (total != P.n_dist || P.mask_words != (uint64_t)n_levels * total || P.sub_words != (uint64_t)n_jobs * n_levels * 64)
        bad("plan sizes", (long long)total, (long long)P.mask_words, (long long)P.sub_words);
    std::vector<uint32_t> rows(P.rows_words);
    std::vector<int32_t> dist(P.n_dist);
    for (uint32_t j = 0; j < n_jobs; j++) {
        const ConsJobDev &J = P.jobs[j];
        const int m = P.len[J.draft];
        if (P.member_off[j] != J.dist_off) bad("member_off", j);
        if (P.agree_off[j + 1] - P.agree_off[j] != (uint64_t)n_levels * (m + 1)) bad("agree_off", j);
        for (uint32_t i = 0; i < J.n; i++) {
            const uint32_t r = J.r0 + i;
            uint32_t *row = rows.data() + J.rows_off + (size_t)i * (m + 1);
            const int d = dp_row(R.seq[J.draft], R.seq[r], row);
            const int k = (R.k[J.draft] < 0 || R.k[r] < 0) ? -1 : std::max(R.k[J.draft], R.k[r]);
            dist[J.dist_off + i] = (k >= 0 && d > k) ? -1 : d;
            if (dist[J.dist_off + i] < 0) {                    // the kernel leaves no row for such a member: junk
                for (int p = 0; p <= m; p++) row[p] = (uint32_t)rng();
                count["members_above_limit"]++;
            }
        }
    }
    // masks: per level one shape -- zero, ones, bit 0, bit 63, a d-subset per replicate, random words
    std::vector<uint64_t> masks(P.mask_words);
    for (uint32_t l = 0; l < n_levels; l++)
        for (uint64_t i = 0; i < total; i++) {
            uint64_t w;
            switch ((l + (uint32_t)(rng() % 3 == 0)) % 7) {
                case 0: w = rng(); break;
                case 1: w = rng() & rng(); break;
                case 2: w = 0; break;
                case 3: w = ~0ull; break;
                case 4: w = 1; break;
                case 5: w = 1ull << 63; break;
                default: w = rng() | rng(); break;
            }
            masks[(uint64_t)l * total + i] = w;
        }
    std::vector<uint64_t> agree(P.agree_off.back(), SENTINEL64);
    std::vector<uint32_t> sub(P.sub_words, SENTINEL32);
    resample_host(P, R.bytes.data(), R.off.data(), n_levels, rows.data(), dist.data(), masks.data(), agree.data(), sub.data());
    // ---- plain loops: every replicate's vote table, then the rule
    for (uint32_t j = 0; j < n_jobs; j++) {
        const smx_cons_job &J = jobs[j];
        const ConsJobDev &D = P.jobs[j];
        const Seq &draft = R.seq[J.draft];
        const int m = (int)draft.size();
        count["jobs"]++;
        if (J.n == 0) count["jobs_without_members"]++;
        for (uint32_t l = 0; l < n_levels; l++)
            for (unsigned b = 0; b < 64; b++) {
                std::vector<uint32_t> table((size_t)(m + 1) * SMX_CONS_VOTE_WORDS, 0);
                uint32_t n_b = 0;
                for (uint32_t i = 0; i < J.n; i++) {
                    if (dist[D.dist_off + i] < 0) continue;
                    if (!((masks[(uint64_t)l * total + D.dist_off + i] >> b) & 1)) continue;
                    n_b++;
                    for (int p = 0; p <= m; p++) {
                        uint32_t v[SMX_CONS_VOTE_WORDS] = {0};
                        cons_vote_word(rows[D.rows_off + (size_t)i * (m + 1) + p], v);
                        for (int x = 0; x < SMX_CONS_VOTE_WORDS; x++) table[(size_t)p * SMX_CONS_VOTE_WORDS + x] += v[x];
                    }
                }
                if (sub[((size_t)j * n_levels + l) * 64 + b] != n_b) bad("sub_aligned", j, l, b);
                if (n_b == 0) count["empty_replicates"]++;
                bool all = true;
                for (int p = 0; p <= m; p++) {
                    const uint32_t *v = table.data() + (size_t)p * SMX_CONS_VOTE_WORDS;
                    const unsigned dc = p < m ? code_of((unsigned char)draft[p]) : 4;
                    const bool want = ref_keeps_as_written(v, n_b, dc, p == m);
                    if (want != ref_keeps_by_call(v, n_b, dc, p == m)) bad("the two references", j, l, p);
                    const bool got = (agree[P.agree_off[j] + (size_t)l * (m + 1) + p] >> b) & 1;
                    if (got != want) bad("agree bit", j, l, p);
                    count["bits"]++;
                    all = all && want;
                    if (!want) {
                        count["bits_clear"]++;
                        if (p == 0) count["clear_at_0"]++;
                        if (p == m - 1) count["clear_at_m_minus_1"]++;
                        if (p == m) count["clear_at_m"]++;
                        if (p < m && dc == 4) count["clear_on_other_draft"]++;
                    }
                }
                if (all) count["replicates_all_kept"]++;
            }
    }
}

static void run_random(uint64_t seed) {
    std::mt19937_64 rng(seed * 0x9E3779B97F4A7C15ull + 31);
    auto uni = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    auto rand_seq = [&](int n) { Seq s(n, 'A'); for (char &c : s) c = "ACGT"[rng() % 4]; return s; };
    auto mutate = [&](const Seq &s, int per_mille) {
        Seq out;
        for (char c : s) {
            const int r = (int)(rng() % 1000);
            if (r < per_mille) out.push_back("ACGTN"[rng() % 5]);
            else if (r < 2 * per_mille) { out.push_back(c); out.push_back("ACGT"[rng() % 4]); }
            else if (r >= 3 * per_mille) out.push_back(c);
        }
        return out;
    };
    const std::vector<int> sizes = {1, 2, 0, 63, 64, 65, 5, 129, 200, 0, 20};
    const std::vector<int> lens = {1, 2, 5, 63, 64, 65, 255, 256, 257, 300};
    const std::vector<uint32_t> levels = {1, 2, 16, 3, 8};
    int made = 0;
    for (int call = 0; call < 12; call++) {
        Reads R;
        std::vector<smx_cons_job> jobs;
        const int n_jobs = call == 0 ? 1 : uni(2, 7);
        for (int g = 0; g < n_jobs; g++, made++) {
            const int m = made < (int)lens.size() ? lens[made] : uni(1, 120);
            const int n = sizes[made % sizes.size()];
            Seq draft = rand_seq(m);
            if (made % 4 == 1) draft[uni(0, m - 1)] = 'N';                      // a draft byte that is no base
            // a second allele: substitutions at the ends and inside, an extra base behind the last one or before the first
            Seq other = draft;
            for (int p : {0, m - 1, uni(0, m - 1)}) other[p] = other[p] == 'A' ? 'C' : 'A';
            if (m > 8) { other.erase(other.begin() + m / 2); other.insert(other.begin() + m / 3, 'G'); }
            if (made % 3 != 0) other.push_back(other.back() == 'G' ? 'T' : 'G');
            if (made % 5 == 0) other.insert(other.begin(), "ACGT"[rng() % 4]);
            const uint32_t r0 = (uint32_t)R.k.size();
            for (int i = 0; i < n; i++) {
                const int kind = (int)(rng() % 8);
                Seq s = mutate(kind < 4 ? other : draft, made % 2 ? 30 : 0);
                int k = kind == 7 ? -1 : m / 5 + 3;
                if (kind == 6) { s = rand_seq(m + 30); k = m / 10; }           // above its limit
                R.add(s, k);
            }
            const uint32_t d = R.add(draft, m / 5 + 3);                         // the draft is not a member
            jobs.push_back(smx_cons_job{d, r0, (uint32_t)n});
        }
        check_call(R, jobs, levels[call % levels.size()], rng);
        count["calls"]++;
    }
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "exhaustive")) {
        run_exhaustive();
    } else if (argc >= 3 && !strcmp(argv[1], "random")) {
        run_random(strtoull(argv[2], nullptr, 10));
    } else {
        fprintf(stderr, "usage: resample_sim exhaustive | random <seed>\n");
        return 2;
    }
    for (auto &kv : count) printf("%s %lld\n", kv.first.c_str(), kv.second);
    printf("%lld mismatches\n", mismatches);
    return 0;
}
