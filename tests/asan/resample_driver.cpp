// AddressSanitizer / UBSan driver for the host side of smx_cons_resample: the plan of a call with its resampling tables
// (smx_cons_plan.h: cons_plan, then cons_plan_resample -- argument checks and the offsets of the mask and agree words)
// and the kernel's body as a host loop (tests/cpu/resample_host.h over smx_resample_core.h) run over the plan's jobs the
// way smx_resample.hip indexes them, with buffers of exactly the planned sizes, so that any index the plan did not budget
// for is a heap overflow.  The rows come from the banded alignment itself (smx_cons_core.h, host build).  CPU only; built
// and run by tests/test_resample_asan.py with g++ -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../cpu/resample_host.h"

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
    std::mt19937 rng(11);
    std::mt19937_64 rng64(12);
    Reads R;
    std::vector<smx_cons_job> jobs;
    // jobs of 1, 63, 64, 65 and 129 members around short drafts with a second allele, the last member of each above its
    // limit, a job without members in the middle; the drafts are no members
    for (int n : {1, 63, 0, 64, 65, 129}) {
        const int m = 40 + n % 7;
        const std::string q = rand_seq(rng, m);
        std::string other = q;
        other[0] = other[0] == 'A' ? 'C' : 'A';
        other[m - 1] = other[m - 1] == 'A' ? 'C' : 'A';
        other.push_back('G');
        const int k = m / 5 + 3;
        const uint32_t r0 = (uint32_t)R.k.size();
        for (int i = 0; i < n; i++) R.add(i + 1 == n && n > 1 ? rand_seq(rng, m + 30) : mutate(rng, i % 2 ? q : other, 10), k);
        const uint32_t d = R.add(q, k);
        jobs.push_back(smx_cons_job{d, r0, (uint32_t)n});
    }
    const uint32_t n_reads = (uint32_t)R.k.size(), n_jobs = (uint32_t)jobs.size();
    ConsPlan P;
    std::string why;
    if (cons_plan(R.bytes.data(), R.off.data(), n_reads, R.k.data(), jobs.data(), n_jobs, CONS_HIST_BYTES, &P, &why) != SMX_OK)
        die(why.c_str());
    // what the resampling plan must refuse, and what it must not
    if (cons_plan_resample(true, 0, &P, &why) != SMX_ERR_ARG || why.find("n_levels") == std::string::npos) die("n_levels = 0 was accepted");
    if (cons_plan_resample(true, SMX_CONS_MAX_LEVELS + 1, &P, &why) != SMX_ERR_ARG) die("n_levels = 17 was accepted");
    if (cons_plan_resample(false, 4, &P, &why) != SMX_ERR_ARG || why.find("masks") == std::string::npos) die("null masks were accepted");
    {
        ConsPlan E;
        if (cons_plan(R.bytes.data(), R.off.data(), n_reads, R.k.data(), jobs.data(), 0, CONS_HIST_BYTES, &E, &why) != SMX_OK) die(why.c_str());
        if (cons_plan_resample(true, 0, &E, &why) != SMX_ERR_ARG) die("n_levels = 0 was accepted where there is no job");
        if (cons_plan_resample(false, 1, &E, &why) != SMX_OK || E.mask_words || E.sub_words || E.agree_off.back()) die("the empty call");
    }
    // align once: the rows and distances every level count reads
    std::vector<uint32_t> rows(P.rows_words);
    std::vector<int32_t> dist(P.n_dist);
    std::vector<cons_pm> hpm(P.hist_slice * MINE_THREADS);
    std::vector<int> hs(P.hist_slice * MINE_THREADS);
    std::vector<mine_u4> tbuf;
    long long above = 0;
    for (uint32_t j = 0; j < n_jobs; j++) {
        const ConsJobDev &J = P.jobs[j];
        const int m = P.len[J.draft];
        const Query Q(R.bytes.data() + R.off[J.draft], m);
        if (Q.W != 1) die("the drafts of this driver have one word");
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
            above += dist[J.dist_off + i] < 0;
        }
    }
    long long words = 0, set = 0, clear = 0, voters = 0;
    for (uint32_t n_levels : {1u, 3u, (uint32_t)SMX_CONS_MAX_LEVELS}) {
        if (cons_plan_resample(true, n_levels, &P, &why) != SMX_OK) die(why.c_str());
        if (P.member_off.size() != (size_t)n_jobs + 1 || P.agree_off.size() != (size_t)n_jobs + 1) die("offsets do not have n_jobs + 1 entries");
        if (P.member_off.back() != P.n_dist) die("the members of the plan are not the members of the call");
        // buffers of exactly the planned sizes
        std::vector<uint64_t> masks(P.mask_words), agree(P.agree_off.back(), 0xDEADBEEFDEADBEEFull);
        std::vector<uint32_t> sub(P.sub_words, 0xDEADBEEFu);
        for (uint64_t &w : masks) w = rng64() | (rng64() & rng64());
        resample_host(P, R.bytes.data(), R.off.data(), n_levels, rows.data(), dist.data(), masks.data(), agree.data(), sub.data());
        for (uint32_t j = 0; j < n_jobs; j++) {
            const uint64_t per_level = (uint64_t)P.len[P.jobs[j].draft] + 1;
            if (P.agree_off[j] + n_levels * per_level != P.agree_off[j + 1]) die("a job's agree words do not end where the next job's begin");
            for (uint64_t w = P.agree_off[j]; w < P.agree_off[j + 1]; w++) {
                if (P.jobs[j].n == 0 && agree[w] != ~0ull) die("the job without members does not keep every column");
                set += __builtin_popcountll(agree[w]);
                clear += 64 - __builtin_popcountll(agree[w]);
                words++;
            }
            for (uint32_t x = 0; x < n_levels * 64; x++) {
                const uint32_t v = sub[((size_t)j * n_levels) * 64 + x];
                if (v > P.jobs[j].n) die("a replicate has more voters than the job has members");
                voters += v;
            }
        }
    }
    if (dist[P.jobs[1].dist_off + 62] != -1) die("the last member of the second job is within its limit");
    printf("jobs %u words %lld set %lld clear %lld voters %lld above %lld\n", n_jobs, words, set, clear, voters, above);
    return 0;
}
