// AddressSanitizer / UBSan driver for the host side of smx_cons_profile: the plan of a call with its profile tables
// (smx_cons_plan.h: cons_plan, then cons_plan_profile -- argument checks, the sizes of the member words and job tables,
// the launch) and the kernel's body as a host loop (tests/cpu/profile_host.h over smx_profile_core.h) run over the plan's
// jobs the way smx_profile.hip indexes them, with buffers of exactly the planned sizes, so that any index the plan did not
// budget for -- a row word, a draft byte, a quality byte, a member word -- is a heap overflow.  The rows come from the
// banded alignment itself (smx_cons_core.h, host build).  CPU only; built and run by tests/test_profile_asan.py with
// g++ -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../cpu/profile_host.h"

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

static std::string rand_seq(std::mt19937 &rng, int n) {          // with runs, and an `N` now and then
    std::string s;
    while ((int)s.size() < n) s.append(rng() % 3 ? 1 : 2 + rng() % 9, "ACGTN"[rng() % 41 ? rng() % 4 : 4]);
    s.resize(n);
    return s;
}

static std::string mutate(std::mt19937 &rng, const std::string &s, int per_mille) {
    std::string out;
    for (char c : s) {
        const int r = (int)(rng() % 1000);
        if (r < per_mille) out.push_back("ACGT"[rng() % 4]);
        else if (r < 2 * per_mille) { out.push_back(c); out.append(1 + rng() % 6, rng() % 2 ? c : "ACGT"[rng() % 4]); }
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
    std::mt19937 rng(21);
    Reads R;
    std::vector<smx_cons_job> jobs;
    // jobs of 1, 16, 0, 17, 4, 5 and 65 members around drafts of 63 .. 129 bases: the last member of each larger job is
    // above its limit, one member carries an insertion that is clipped, one is empty; the drafts are no members
    const int lens[] = {63, 64, 65, 127, 128, 129, 100};
    int g = 0;
    for (int n : {1, 16, 0, 17, 4, 5, 65}) {
        const int m = lens[g++];
        const std::string q = rand_seq(rng, m);
        const uint32_t r0 = (uint32_t)R.k.size();
        for (int i = 0; i < n; i++) {
            std::string s = mutate(rng, q, 30);
            int k = m;                                        // a mutated read is always within it
            if (i + 1 == n && n > 4) { s = rand_seq(rng, m + 30); k = 3; }
            else if (i == 2) { s.insert(s.size() / 2, 256 + rng() % 10, 'T'); k = -1; }
            else if (i == 3) { s.clear(); k = -1; }
            R.add(s, k);
        }
        const uint32_t d = R.add(q, 3);
        jobs.push_back(smx_cons_job{d, r0, (uint32_t)n});
    }
    const uint32_t n_reads = (uint32_t)R.k.size(), n_jobs = (uint32_t)jobs.size();
    ConsPlan P;
    std::string why;
    if (cons_plan(R.bytes.data(), R.off.data(), n_reads, R.k.data(), jobs.data(), n_jobs, CONS_HIST_BYTES, &P, &why) != SMX_OK)
        die(why.c_str());
    // what the profile plan must refuse, and what it must not
    if (cons_plan_profile(false, true, true, &P, &why) != SMX_ERR_ARG || why.find("quals") == std::string::npos) die("null quals were accepted");
    if (cons_plan_profile(true, false, true, &P, &why) != SMX_ERR_ARG || why.find("per_member") == std::string::npos) die("null per_member was accepted");
    if (cons_plan_profile(true, true, false, &P, &why) != SMX_ERR_ARG || why.find("tables") == std::string::npos) die("null tables were accepted");
    {
        ConsPlan E;                                            // no job has members: nothing is needed, nothing launched
        const smx_cons_job none{jobs[2].draft, jobs[2].r0, 0};
        if (cons_plan(R.bytes.data(), R.off.data(), n_reads, R.k.data(), &none, 1, CONS_HIST_BYTES, &E, &why) != SMX_OK) die(why.c_str());
        if (cons_plan_profile(false, false, false, &E, &why) != SMX_OK || E.member_words || E.profile_max_members ||
            E.table_words != SMX_PROFILE_JOB_WORDS)
            die("the call without members");
        ConsPlan B = E;                                        // more members than a grid dimension holds times the slice
        B.jobs[0].n = SMX_PROFILE_BLOCK_MEMBERS * 65535u + 1u;
        if (cons_plan_profile(true, true, true, &B, &why) != SMX_ERR_UNSUPPORTED || why.find("split the call") == std::string::npos)
            die("a job beyond the launch was accepted");
        B.jobs[0].n = SMX_PROFILE_BLOCK_MEMBERS * 65535u;
        if (cons_plan_profile(true, true, true, &B, &why) != SMX_OK) die("the largest job a launch holds was refused");
    }
    if (cons_plan_profile(true, true, true, &P, &why) != SMX_OK) die(why.c_str());
    if (P.member_words != P.n_dist * SMX_PROFILE_MEMBER_WORDS || P.table_words != (uint64_t)n_jobs * SMX_PROFILE_JOB_WORDS ||
        P.profile_max_members != 65)
        die("the planned sizes");
    // align: the rows and distances the kernel reads
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
        if (Q.W > 4) die("the drafts of this driver have four words at most");
        for (uint32_t i = 0; i < J.n; i++) {
            const uint32_t r = J.r0 + i;
            const int n = P.len[r], lane = (int)((i * 37 + 127) % MINE_THREADS);
            tbuf.assign((size_t)n / 16 + 1, mine_u4{0, 0, 0, 0});
            memcpy(tbuf.data(), R.bytes.data() + R.off[r], (size_t)n);
            const int k = (R.k[J.draft] < 0 || R.k[r] < 0) ? -1 : std::max(R.k[J.draft], R.k[r]);
            const ConsHist H{hpm.data() + lane, hs.data() + lane, (int)J.B};
            RegState<4> st;
            dist[J.dist_off + i] = cons_pair<4>(st, H, Q.peq.data(), Q.rowmap, Q.m, Q.W, Q.Wp, k,
                                                reinterpret_cast<const unsigned char *>(tbuf.data()), n,
                                                rows.data() + J.rows_off + (size_t)i * (m + 1));
            above += dist[J.dist_off + i] < 0;
        }
    }
    // buffers of exactly the planned sizes; the quality bytes take every value
    std::vector<unsigned char> quals(R.bytes.size());
    for (unsigned char &b : quals) b = (unsigned char)(rng() % 256);
    std::vector<uint32_t> per_member(P.member_words, 0xDEADBEEFu), tables(P.table_words, 0u);
    profile_host(P, R.bytes.data(), R.off.data(), rows.data(), dist.data(), quals.data(), per_member.data(), tables.data());
    long long members = 0, clipped = 0, q_bases = 0, read_bases = 0, columns = 0, hp = 0, empty = 0;
    for (uint32_t j = 0; j < n_jobs; j++) {
        const ConsJobDev &J = P.jobs[j];
        const uint32_t m = (uint32_t)P.len[J.draft];
        const uint32_t *t = tables.data() + (size_t)j * SMX_PROFILE_JOB_WORDS;
        for (uint32_t i = 0; i < J.n; i++) {
            const uint32_t *w = per_member.data() + (J.dist_off + i) * SMX_PROFILE_MEMBER_WORDS;
            if (dist[J.dist_off + i] < 0) {
                for (int x = 0; x < 8; x++) if (w[x]) die("a member above its limit has counts");
                continue;
            }
            if (w[0] + w[1] + w[2] + w[3] != m || w[6] > 1 || w[7]) die("a member's columns do not add up to the draft");
            const uint32_t len = (uint32_t)P.len[J.r0 + i];
            if (!w[6] && w[0] + w[1] + w[3] + w[5] != len) die("an unclipped member's bases do not add up to the read");
            members++, clipped += w[6], columns += m, empty += len == 0;
            if (!w[6]) read_bases += len;
        }
        for (unsigned x = 0; x < PROFILE_Q_WORDS; x++) q_bases += t[x];
        for (unsigned x = PROFILE_HP; x < SMX_PROFILE_JOB_WORDS; x++) hp += t[x];
        if (J.n == 0) for (unsigned x = 0; x < SMX_PROFILE_JOB_WORDS; x++) if (t[x]) die("the job without members has counts");
    }
    if (q_bases != read_bases) die("the q table does not hold every base of the unclipped members once");
    printf("jobs %u members %lld above %lld clipped %lld empty %lld columns %lld q_bases %lld hp %lld\n", n_jobs, members, above, clipped,
           empty, columns, q_bases, hp);
    return 0;
}
