// AddressSanitizer / UBSan driver for the host side of smx_cons_phase: the plan of a call with its variant tables
// (smx_cons_plan.h: cons_plan, then cons_plan_phase -- argument checks and the offsets of sites, planes and link) and the
// shared core (smx_cons_core.h, smx_phase_core.h, host build) run over the plan's jobs the way the kernels of smx_phase.hip
// index them, with buffers of exactly the planned sizes, so that any index the plan did not budget for is a heap
// overflow.  CPU only; built and run by tests/test_phase_asan.py with g++ -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "smx_cons_plan.h"
#include "smx_phase_core.h"

using namespace smx;

static void die(const char *what) { fprintf(stderr, "driver: %s\n", what); exit(2); }

struct Reads {
    std::string bytes;
    std::vector<uint64_t> off{0};
    std::vector<int32_t> k;
    uint32_t add(const std::string &s, int kk) {
        bytes += s;
        off.push_back(bytes.size());
        k.push_back(kk);
        return (uint32_t)k.size() - 1;
    }
};

static std::string rand_seq(std::mt19937 &rng, int n) {
    std::string s(n, 'A');
    for (char &c : s) c = "ACGTN"[rng() % 5];
    return s;
}

static std::string mutate(std::mt19937 &rng, const std::string &s, int per_mille) {
    std::string out;
    for (char c : s) {
        const int r = (int)(rng() % 1000);
        if (r < per_mille) out.push_back("ACGT"[rng() % 4]);
        else if (r < 2 * per_mille) { out.push_back(c); out.push_back("ACGT"[rng() % 4]); }
        else if (r >= 3 * per_mille) out.push_back(c);
    }
    return out;
}

// the draft's Peq table as mine_build_peq leaves it
struct Query {
    int m, W, Wp;
    unsigned short rowmap[256];
    std::vector<u64> peq;
    Query(const char *q, int len) : m(len), W((len + 63) >> 6), Wp(W | 1) {
        bool present[256] = {false};
        for (int i = 0; i < m; i++) present[(unsigned char)q[i]] = true;
        int base = 1;
        for (int c = 0; c < 256; c++) rowmap[c] = present[c] ? (unsigned short)base++ : (unsigned short)0;
        peq.assign((size_t)base * Wp, 0ull);
        for (int i = 0; i < m; i++) peq[(size_t)rowmap[(unsigned char)q[i]] * Wp + (i >> 6)] |= 1ull << (i & 63);
    }
};

int main() {
    std::mt19937 rng(7);
    Reads R;
    std::vector<smx_cons_job> jobs;
    // jobs of 1, 63, 64, 65 and 129 members (the plane-word edges) around short drafts with a second allele, the last
    // member of each above its limit; then a job without members
    for (int n : {1, 63, 64, 65, 129}) {
        const int m = 40 + n % 7;
        const std::string q = rand_seq(rng, m);
        std::string other = q;
        other[0] = other[0] == 'A' ? 'C' : 'A';
        other[m / 2] = other[m / 2] == 'A' ? 'C' : 'A';
        other.push_back('G');
        const int k = m / 5 + 3;
        const uint32_t r0 = R.add(q, k);
        for (int i = 1; i < n; i++) R.add(i + 1 == n ? rand_seq(rng, m + 30) : mutate(rng, i % 3 ? q : other, 10), k);
        jobs.push_back(smx_cons_job{r0, r0, (uint32_t)n});
    }
    jobs.push_back(smx_cons_job{0, 1, 0});
    const uint32_t n_reads = (uint32_t)R.k.size(), n_jobs = (uint32_t)jobs.size();
    ConsPlan P;
    std::string why;
    if (cons_plan(R.bytes.data(), R.off.data(), n_reads, R.k.data(), jobs.data(), n_jobs, CONS_HIST_BYTES, &P, &why) != SMX_OK)
        die(why.c_str());
    // what the variant plan must refuse
    if (cons_plan_phase(150, 0, &P, &why) != SMX_ERR_ARG) die("max_sites = 0 was accepted");
    if (cons_plan_phase(150, SMX_CONS_MAX_SITES + 1, &P, &why) != SMX_ERR_ARG) die("max_sites = 65 was accepted");
    if (cons_plan_phase(1001, 8, &P, &why) != SMX_ERR_ARG) die("min_permille = 1001 was accepted");
    long long kept_total = 0, clipped = 0, checksum = 0, bits = 0;
    for (uint32_t max_sites : {1u, 3u, (uint32_t)SMX_CONS_MAX_SITES}) {
        const uint32_t min_permille = 20, min_reads = 2;      // low enough for the noise to add sites of its own
        if (cons_plan_phase(min_permille, max_sites, &P, &why) != SMX_OK) die(why.c_str());
        if (P.planes_off.size() != (size_t)n_jobs + 1) die("planes_off does not have n_jobs + 1 entries");
        // buffers of exactly the planned sizes
        std::vector<uint32_t> rows(P.rows_words), votes(P.votes_words), aligned(n_jobs), n_sites(n_jobs), n_qualified(n_jobs);
        std::vector<int32_t> dist(P.n_dist);
        std::vector<cons_pm> hpm(P.hist_slice * MINE_THREADS);
        std::vector<int> hs(P.hist_slice * MINE_THREADS);
        std::vector<smx_cons_site> sites(P.site_slots);
        std::vector<uint64_t> planes(P.planes_off.back());
        std::vector<uint32_t> link(P.link_words);
        std::vector<mine_u4> tbuf;
        for (uint32_t j = 0; j < n_jobs; j++) {
            const ConsJobDev &J = P.jobs[j];
            const int m = P.len[J.draft];
            const Query Q(R.bytes.data() + R.off[J.draft], m);
            if (Q.W != 1) die("the drafts of this driver have one word");
            // ---- align and vote, as the kernels of smx_cons.hip do
            for (uint32_t i = 0; i < J.n; i++) {
                const uint32_t r = J.r0 + i;
                const int n = P.len[r], lane = (int)((i * 37 + 127) % MINE_THREADS);
                tbuf.assign((size_t)n / 16 + 1, mine_u4{0, 0, 0, 0});
                memcpy(tbuf.data(), R.bytes.data() + R.off[r], (size_t)n);
                const int k = (R.k[J.draft] < 0 || R.k[r] < 0) ? -1 : std::max(R.k[J.draft], R.k[r]);
                const ConsHist H{hpm.data() + lane, hs.data() + lane, (int)J.B};
                RegState<1> st;
                dist[J.dist_off + i] = cons_pair<1>(st, H, Q.peq.data(), Q.rowmap, Q.m, Q.W, Q.Wp, k,
                                                    reinterpret_cast<const unsigned char *>(tbuf.data()), n,
                                                    rows.data() + J.rows_off + (size_t)i * (m + 1));
            }
            for (int p = 0; p <= m; p++) {
                uint32_t v[SMX_CONS_VOTE_WORDS] = {0};
                for (uint32_t i = 0; i < J.n; i++)
                    if (dist[J.dist_off + i] >= 0) cons_vote_word(rows[J.rows_off + (size_t)i * (m + 1) + p], v);
                memcpy(votes.data() + J.votes_off + (size_t)p * SMX_CONS_VOTE_WORDS, v, sizeof v);
            }
            for (uint32_t i = 0; i < J.n; i++) aligned[j] += dist[J.dist_off + i] >= 0;
            // ---- phase_sites_kernel
            smx_cons_site *out = sites.data() + (size_t)j * max_sites;
            uint32_t base = 0;
            for (int p = 0; J.n != 0 && p <= m; p++) {
                const uint32_t *v = votes.data() + J.votes_off + (size_t)p * SMX_CONS_VOTE_WORDS;
                const smx_cons_site a = phase_ins_site(v, (uint32_t)p, aligned[j]);
                if (phase_qualifies(a.n_minor, aligned[j], min_reads, min_permille)) { if (base < max_sites) out[base] = a; base++; }
                if (p == m) break;
                const smx_cons_site b = phase_base_site(v, (uint32_t)p);
                if (phase_qualifies(b.n_minor, aligned[j], min_reads, min_permille)) { if (base < max_sites) out[base] = b; base++; }
            }
            n_sites[j] = std::min(base, max_sites);
            n_qualified[j] = base;
            for (uint32_t s = n_sites[j]; s < max_sites; s++) out[s] = phase_make_site(0, 0, 0, 0, 0, 0);
            // ---- phase_planes_kernel: a wave per word, a lane per member
            const uint32_t words = (J.n + 63) / 64;
            uint64_t *pl = planes.data() + P.planes_off[j];
            for (uint32_t word = 0; word < words; word++)
                for (uint32_t s = 0; s < max_sites; s++) {
                    uint64_t minor = 0, major = 0;
                    for (uint32_t lane = 0; lane < 64 && s < n_sites[j]; lane++) {
                        const uint32_t member = word * 64 + lane;
                        if (member >= J.n || dist[J.dist_off + member] < 0) continue;
                        const unsigned c = phase_classify(rows[J.rows_off + (size_t)member * (m + 1) + out[s].pos], out[s].kind,
                                                          out[s].major, out[s].minor);
                        minor |= (uint64_t)(c == PHASE_MINOR) << lane;
                        major |= (uint64_t)(c == PHASE_MAJOR) << lane;
                    }
                    pl[(size_t)(2 * s) * words + word] = minor;
                    pl[(size_t)(2 * s + 1) * words + word] = major;
                    bits += phase_popc(minor) + phase_popc(major);
                }
            if (P.planes_off[j] + (uint64_t)max_sites * 2 * words != P.planes_off[j + 1]) die("a job's plane words do not end where the next job's begin");
            // ---- phase_link_kernel: every entry of the job's table
            uint32_t *lk = link.data() + (size_t)j * max_sites * max_sites * 4;
            for (uint32_t e = 0; e < max_sites * max_sites; e++) {
                const uint32_t s = e / max_sites, t = e % max_sites;
                uint32_t c[4] = {0, 0, 0, 0};
                if (s < t && t < n_sites[j])
                    for (uint32_t w = 0; w < words; w++)
                        phase_link_word(pl[(size_t)(2 * s) * words + w], pl[(size_t)(2 * s + 1) * words + w],
                                        pl[(size_t)(2 * t) * words + w], pl[(size_t)(2 * t + 1) * words + w], c);
                memcpy(lk + (size_t)e * 4, c, sizeof c);
                checksum += c[0] + 2 * c[1] + 3 * c[2] + 5 * c[3];
            }
            kept_total += n_sites[j];
            clipped += n_qualified[j] > n_sites[j];
        }
        if (n_sites[n_jobs - 1] != 0 || n_qualified[n_jobs - 1] != 0) die("the job without members has sites");
        if (dist[P.jobs[1].dist_off + 62] != -1) die("the last member of the second job is within its limit");
    }
    printf("jobs %u kept %lld clipped %lld bits %lld checksum %lld\n", n_jobs, kept_total, clipped, bits, checksum);
    return 0;
}
