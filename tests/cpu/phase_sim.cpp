// CPU simulation of the variant kernels' shared code (specimux_amd/csrc/smx_phase_core.h): the same host/device
// functions smx_phase.hip runs -- the site rule over a vote table, the classification of a row word at a site, the plane
// words and the link counts -- checked against plain loops over pileup rows.  The rows come from the full-matrix
// reference walk of tests/cpu/cons_sim.cpp (dp_row below is that function: NW over the whole matrix, then the fixed walk
// diagonal, else up, else left), not from the banded code under test there.  Built and run by tests/test_phase_cpu.py
// (g++, no GPU).
//
//   phase_sim exhaustive        every vote vector in {0..3}^6 for the base rule, every (present, aligned <= 12) for the
//                               insertion rule, every (n_minor, aligned <= 40, min_reads <= 3, min_permille) around the
//                               threshold for the qualification, every row word field for the classification
//   phase_sim random <seed>     jobs of 1..200 members around drafts of 1..320 nt with planted alleles, members above
//                               their limit, `N` bytes and indels on and next to the sites
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

#include "smx_cons_core.h"    // cons_vote_word: the vote table as the vote kernel fills it
#include "smx_phase_core.h"

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
static int dp_row(const Seq &q, const Seq &t, std::vector<uint32_t> *row_out) {
    const int m = (int)q.size(), n = (int)t.size();
    std::vector<int> D((size_t)(m + 1) * (n + 1));
    auto at = [&](int i, int j) -> int & { return D[(size_t)i * (n + 1) + j]; };
    for (int i = 0; i <= m; i++) at(i, 0) = i;
    for (int j = 0; j <= n; j++) at(0, j) = j;
    for (int i = 1; i <= m; i++)
        for (int j = 1; j <= n; j++)
            at(i, j) = std::min(std::min(at(i - 1, j) + 1, at(i, j - 1) + 1), at(i - 1, j - 1) + (q[i - 1] != t[j - 1]));
    std::vector<uint32_t> &row = *row_out;
    row.assign(m + 1, 0);
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

// ---- the rules again, written as plain loops
struct RefSite { uint32_t pos; unsigned kind, major, minor; uint32_t n_major, n_minor; };

static bool same(const smx_cons_site &a, const RefSite &b) {
    return a.pos == b.pos && a.kind == b.kind && a.major == b.major && a.minor == b.minor && a.n_major == b.n_major &&
           a.n_minor == b.n_minor && a.pad == 0;
}

// the base site of the symbol counts n[A, C, G, T, other, deletion]: most and second most of A C G T deletion, by a stable
// sort on the count (descending) of the codes in ascending order
static RefSite ref_base(const uint32_t *sym, uint32_t p) {
    std::vector<unsigned> codes = {0, 1, 2, 3, 5};
    std::stable_sort(codes.begin(), codes.end(), [&](unsigned a, unsigned b) { return sym[a] > sym[b]; });
    return RefSite{p, 0, codes[0], codes[1], sym[codes[0]], sym[codes[1]]};
}

static RefSite ref_ins(uint32_t present, uint32_t aligned, uint32_t p) {
    const uint32_t absent = aligned - present;
    if (present < absent || present == absent) return RefSite{p, 1, 0, 1, absent, present};
    return RefSite{p, 1, 1, 0, present, absent};
}

// n_minor / aligned >= min_permille / 1000 in exact rationals, and the count floor
static bool ref_qualifies(uint32_t n_minor, uint32_t aligned, uint32_t min_reads, uint32_t min_permille) {
    if (n_minor < min_reads) return false;
    return (unsigned long long)n_minor * 1000ull >= (unsigned long long)min_permille * aligned;
}

// 0 neither, 1 minor, 2 major: what the member of this row has at the site, from the row's fields
static unsigned ref_class(uint32_t word, const RefSite &s) {
    unsigned have;
    if (s.kind == 1) have = ((word >> 3) & 0xffu) > 0 ? 1u : 0u;
    else have = word & 7u;
    if (have == s.minor) return 1;
    if (have == s.major) return 2;
    return 0;
}

static void run_exhaustive() {
    // the base rule: every vector of six counts in 0..3 (sym[4] must not matter), ties of every shape
    uint32_t v[SMX_CONS_VOTE_WORDS];
    for (int x = 0; x < 4096; x++) {
        memset(v, 0, sizeof v);
        for (int c = 0; c < 6; c++) v[c] = (uint32_t)((x >> (2 * c)) & 3);
        for (int c = 6; c < SMX_CONS_VOTE_WORDS; c++) v[c] = (uint32_t)(x * 7 + c);   // junk the base rule must not read
        const smx_cons_site got = phase_base_site(v, (uint32_t)x);
        const RefSite want = ref_base(v, (uint32_t)x);
        if (!same(got, want)) bad("base", x, got.major, got.minor);
        count["base_vectors"]++;
        if (want.n_major == want.n_minor) count["base_tie_major"]++;
        std::vector<uint32_t> rest;
        for (unsigned c : {0u, 1u, 2u, 3u, 5u})
            if (c != want.major) rest.push_back(v[c]);
        std::sort(rest.rbegin(), rest.rend());
        if (rest[0] == rest[1]) count["base_tie_minor"]++;
        if (v[4] > want.n_major) count["base_other_largest"]++;
    }
    // the insertion rule: present spread over the five codes of slot 0 in every way of two codes
    for (uint32_t aligned = 0; aligned <= 12; aligned++)
        for (uint32_t present = 0; present <= aligned; present++)
            for (uint32_t first = 0; first <= present; first++)
                for (int c0 = 0; c0 < 5; c0++) {
                    memset(v, 0, sizeof v);
                    for (int c = 0; c < 6; c++) v[c] = 1000 + c;              // junk the insertion rule must not read
                    for (int c = 11; c < SMX_CONS_VOTE_WORDS; c++) v[c] = 77; // the later slots
                    v[6 + c0] += first;
                    v[6 + (c0 + 2) % 5] += present - first;
                    const smx_cons_site got = phase_ins_site(v, aligned, aligned);
                    if (!same(got, ref_ins(present, aligned, aligned))) bad("ins", aligned, present, first);
                    count["ins_vectors"]++;
                    if (2 * present == aligned) count["ins_tie"]++;
                }
    // the thresholds: every count around them
    for (uint32_t aligned = 0; aligned <= 40; aligned++)
        for (uint32_t n_minor = 0; n_minor <= aligned; n_minor++)
            for (uint32_t min_reads = 0; min_reads <= 3; min_reads++)
                for (uint32_t pm : {0u, 1u, 100u, 149u, 150u, 151u, 250u, 333u, 334u, 500u, 999u, 1000u}) {
                    const bool got = phase_qualifies(n_minor, aligned, min_reads, pm), want = ref_qualifies(n_minor, aligned, min_reads, pm);
                    if (got != want) bad("qualifies", n_minor, aligned, pm);
                    count["threshold_cases"]++;
                    if ((unsigned long long)n_minor * 1000ull == (unsigned long long)pm * aligned && aligned) count["on_share_threshold"]++;
                    if (n_minor == min_reads) count["on_count_threshold"]++;
                }
    // large counts: the products need 64 bits
    if (!phase_qualifies(3000000000u, 4000000000u, 1, 750) || phase_qualifies(2999999999u, 4000000000u, 1, 750)) bad("qualifies64");
    // the classification: every symbol x insertion length 0 / 1 / 255 x slot junk against every (kind, major, minor)
    for (unsigned symv = 0; symv < 8; symv++)
        for (unsigned len : {0u, 1u, 4u, 255u})
            for (unsigned junk : {0u, 0xfffu}) {
                const uint32_t word = symv | (len << 3) | (junk << 11);
                for (unsigned a : {0u, 1u, 2u, 3u, 5u})
                    for (unsigned b : {0u, 1u, 2u, 3u, 5u}) {
                        if (a == b) continue;
                        const RefSite s{0, 0, a, b, 0, 0};
                        if (phase_classify(word, 0, a, b) != ref_class(word, s)) bad("classify base", word, a, b);
                        count["classified"]++;
                    }
                for (unsigned a : {0u, 1u}) {
                    const RefSite s{0, 1, a, 1 - a, 0, 0};
                    if (phase_classify(word, 1, a, 1 - a) != ref_class(word, s)) bad("classify ins", word, a);
                    count["classified"]++;
                }
            }
}

// One job the way the three kernels see it: votes from the rows of the voters, sites from the votes, plane words from
// the rows, link counts from the plane words -- every step against plain loops over the members.
static void check_job(const Seq &draft, const std::vector<Seq> &members, const std::vector<int> &limit, uint32_t min_permille,
                      uint32_t min_reads, uint32_t max_sites, std::mt19937_64 &rng) {
    const int m = (int)draft.size();
    const uint32_t n = (uint32_t)members.size();
    std::vector<std::vector<uint32_t>> rows(n);
    std::vector<int> dist(n);
    uint32_t aligned = 0;
    std::vector<uint32_t> votes((size_t)(m + 1) * SMX_CONS_VOTE_WORDS, 0);
    for (uint32_t i = 0; i < n; i++) {
        const int d = dp_row(draft, members[i], &rows[i]);
        dist[i] = (limit[i] >= 0 && d > limit[i]) ? -1 : d;
        if (dist[i] < 0) {                         // the kernel leaves no row for such a member: junk, never to be read
            for (uint32_t &w : rows[i]) w = (uint32_t)rng();
            count["members_above_limit"]++;
            continue;
        }
        aligned++;
        for (int p = 0; p <= m; p++) {
            uint32_t v[SMX_CONS_VOTE_WORDS] = {0};
            cons_vote_word(rows[i][p], v);
            for (int x = 0; x < SMX_CONS_VOTE_WORDS; x++) votes[(size_t)p * SMX_CONS_VOTE_WORDS + x] += v[x];
        }
    }
    // ---- sites: the core per position, compacted in order; the reference from plain counts over the rows
    std::vector<smx_cons_site> kept;
    uint32_t qualified = 0;
    std::vector<RefSite> want;
    uint32_t want_qualified = 0;
    for (int p = 0; p <= m && n != 0; p++) {
        const uint32_t *v = votes.data() + (size_t)p * SMX_CONS_VOTE_WORDS;
        const smx_cons_site a = phase_ins_site(v, (uint32_t)p, aligned);
        if (phase_qualifies(a.n_minor, aligned, min_reads, min_permille) && qualified++ < max_sites) kept.push_back(a);
        if (p < m) {
            const smx_cons_site b = phase_base_site(v, (uint32_t)p);
            if (phase_qualifies(b.n_minor, aligned, min_reads, min_permille) && qualified++ < max_sites) kept.push_back(b);
        }
        uint32_t present = 0, sym[6] = {0, 0, 0, 0, 0, 0};
        for (uint32_t i = 0; i < n; i++) {
            if (dist[i] < 0) continue;
            present += ((rows[i][p] >> 3) & 255u) != 0;
            if (p < m) sym[rows[i][p] & 7u]++;
        }
        const RefSite ra = ref_ins(present, aligned, (uint32_t)p);
        if (ref_qualifies(ra.n_minor, aligned, min_reads, min_permille) && want_qualified++ < max_sites) want.push_back(ra);
        if (p < m) {
            const RefSite rb = ref_base(sym, (uint32_t)p);
            if (ref_qualifies(rb.n_minor, aligned, min_reads, min_permille) && want_qualified++ < max_sites) want.push_back(rb);
            if (sym[4]) count["positions_with_other"]++;
        }
    }
    if (qualified != want_qualified || kept.size() != want.size()) bad("site count", qualified, want_qualified, m);
    for (size_t s = 0; s < kept.size() && s < want.size(); s++)
        if (!same(kept[s], want[s])) bad("site", (long long)s, kept[s].pos, want[s].pos);
    count["jobs"]++;
    count["sites_kept"] += (long long)kept.size();
    if (qualified > max_sites) count["jobs_clipped"]++;
    for (const smx_cons_site &s : kept) {
        count[s.kind ? "sites_ins" : "sites_base"]++;
        if (s.kind == 0 && (s.major == 5 || s.minor == 5)) count["sites_deletion"]++;
        if (s.pos == 0) count["sites_at_0"]++;
        if ((int)s.pos == m) count["sites_at_m"]++;
        if ((int)s.pos == m - 1 && s.kind == 0) count["sites_at_m_minus_1"]++;
    }
    // ---- planes: lane = member, a word per 64 of them, as the ballots build it
    const uint32_t words = (n + 63) / 64;
    std::vector<uint64_t> planes((size_t)kept.size() * 2 * words, 0);
    for (size_t s = 0; s < kept.size(); s++)
        for (uint32_t i = 0; i < words * 64; i++) {
            const bool voter = i < n && dist[i] >= 0;
            const unsigned c = voter ? phase_classify(rows[i][kept[s].pos], kept[s].kind, kept[s].major, kept[s].minor) : (unsigned)PHASE_NEITHER;
            if (c == PHASE_MINOR) planes[(2 * s) * words + (i >> 6)] |= 1ull << (i & 63);
            if (c == PHASE_MAJOR) planes[(2 * s + 1) * words + (i >> 6)] |= 1ull << (i & 63);
        }
    std::vector<std::vector<unsigned>> cls(want.size(), std::vector<unsigned>(n, 0));
    for (size_t s = 0; s < want.size(); s++) {
        uint32_t n_minor = 0, n_major = 0;
        for (uint32_t i = 0; i < n; i++) {
            if (dist[i] < 0) continue;
            cls[s][i] = ref_class(rows[i][want[s].pos], want[s]);
            n_minor += cls[s][i] == 1;
            n_major += cls[s][i] == 2;
        }
        // the planes agree with the votes the site was made of
        if (n_minor != want[s].n_minor || n_major != want[s].n_major) bad("plane count", (long long)s, n_minor, n_major);
        if (s >= kept.size()) continue;
        uint32_t pop_minor = 0, pop_major = 0;
        for (uint32_t w = 0; w < words; w++) {
            pop_minor += (uint32_t)phase_popc(planes[(2 * s) * words + w]);
            pop_major += (uint32_t)phase_popc(planes[(2 * s + 1) * words + w]);
        }
        if (pop_minor != n_minor || pop_major != n_major) bad("plane popcount", (long long)s, pop_minor, pop_major);
        for (uint32_t i = 0; i < n; i++) {
            const unsigned got = ((planes[(2 * s) * words + (i >> 6)] >> (i & 63)) & 1) ? 1u : ((planes[(2 * s + 1) * words + (i >> 6)] >> (i & 63)) & 1) ? 2u : 0u;
            if (got != cls[s][i]) bad("plane bit", (long long)s, i, got);
            count["plane_bits"]++;
            if (cls[s][i] == 0 && dist[i] >= 0) count["plane_neither"]++;
        }
    }
    // ---- link: popcounts over the words against a count over the members
    for (size_t s = 0; s < kept.size() && s < want.size(); s++)
        for (size_t t = s + 1; t < kept.size() && t < want.size(); t++) {
            uint32_t got[4] = {0, 0, 0, 0}, ref[4] = {0, 0, 0, 0};
            for (uint32_t w = 0; w < words; w++)
                phase_link_word(planes[(2 * s) * words + w], planes[(2 * s + 1) * words + w], planes[(2 * t) * words + w],
                                planes[(2 * t + 1) * words + w], got);
            for (uint32_t i = 0; i < n; i++) {
                const unsigned a = cls[s][i], b = cls[t][i];
                if (a && b) ref[(a == 2) * 2 + (b == 2)]++;
            }
            if (memcmp(got, ref, sizeof got)) bad("link", (long long)s, (long long)t, got[0]);
            count["link_pairs"]++;
            if (got[0] + got[1] + got[2] + got[3] < aligned) count["link_pairs_with_gaps"]++;
        }
}

static void run_random(uint64_t seed) {
    std::mt19937_64 rng(seed * 0x9E3779B97F4A7C15ull + 29);
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
    std::vector<int> sizes = {1, 2, 63, 64, 65, 127, 128, 129, 200};
    std::vector<int> lens = {1, 2, 5, 63, 64, 65, 255, 256, 257, 300, 320};
    for (int round = 0; round < 60; round++) {
        const int m = round < (int)lens.size() ? lens[round] : uni(1, 320);
        const int n = sizes[round % sizes.size()];
        const Seq draft = rand_seq(m);
        // a second allele: substitutions, a deletion and an insertion at a few positions, the ends among them
        Seq other = draft;
        const bool end_ins = round % 3 == 1;      // an insertion site at p = m: the last base stays, so the walk cannot shift it
        std::vector<int> at = {0, end_ins ? 0 : m - 1, uni(0, m - 1), uni(0, m - 1)};
        for (int p : at) other[p] = other[p] == 'A' ? 'C' : 'A';
        if (m > 8) { other.erase(other.begin() + m / 2); other.insert(other.begin() + m / 3, 'G'); }
        if (end_ins) other.push_back(other.back() == 'G' ? 'T' : 'G');
        if (round % 5 == 0) other.insert(other.begin(), "ACGT"[rng() % 4]);  // and one before p = 0
        std::vector<Seq> members;
        std::vector<int> limit;
        for (int i = 0; i < n; i++) {
            const int kind = (int)(rng() % 8);
            members.push_back(mutate(kind < 3 ? other : draft, round % 2 ? 20 : 0));
            limit.push_back(kind == 7 ? -1 : m / 5 + 3);
            if (kind == 6) { members.back() = rand_seq(m + 30); limit.back() = m / 10; }   // above its limit
        }
        static const uint32_t pms[] = {0, 100, 150, 250, 400};
        static const uint32_t sites[] = {1, 2, 3, 8, 32, 64};
        check_job(draft, members, limit, pms[round % 5], (uint32_t)(round % 4), sites[round % 6], rng);
    }
    check_job(rand_seq(40), {}, {}, 0, 0, 8, rng);            // a job without members: no sites, whatever the thresholds
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "exhaustive")) {
        run_exhaustive();
    } else if (argc >= 3 && !strcmp(argv[1], "random")) {
        run_random(strtoull(argv[2], nullptr, 10));
    } else {
        fprintf(stderr, "usage: phase_sim exhaustive | random <seed>\n");
        return 2;
    }
    for (auto &kv : count) printf("%s %lld\n", kv.first.c_str(), kv.second);
    printf("%lld mismatches\n", mismatches);
    return 0;
}
