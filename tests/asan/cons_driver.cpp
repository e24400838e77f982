// AddressSanitizer / UBSan driver for the host side of the consensus calls: the plan of a call (smx_cons_plan.h:
// argument checks, offsets, class lists, history size) and the per-pair code (smx_cons_core.h, host build) run over
// the plan's jobs with buffers of exactly the planned sizes -- the history slice, the rows, the distances and the vote
// table -- so that any index the plan did not budget for is a heap overflow.  CPU only; built and run by
// tests/test_cons_asan.py with g++ -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../cpu/chunk_walk_host.h"   // chunk_with_wr
#include "smx_cons_plan.h"

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

template <int WR>
static int pair_in_class(const ConsHist &H, const Query &Q, int k, const unsigned char *t, int n, uint32_t *row,
                         std::vector<u64> &sP, std::vector<u64> &sM, std::vector<int> &sS, int lane) {
    if (WR > 0) {
        RegState<WR> st;
        return cons_pair<WR>(st, H, Q.peq.data(), Q.rowmap, Q.m, Q.W, Q.Wp, k, t, n, row);
    }
    GlobalState st{sP.data() + lane, sM.data() + lane, sS.data() + lane};
    return cons_pair<0>(st, H, Q.peq.data(), Q.rowmap, Q.m, Q.W, Q.Wp, k, t, n, row);
}

int main() {
    std::mt19937 rng(5);
    Reads R;
    std::vector<smx_cons_job> jobs;
    // drafts of every state class; members: the draft, mutated copies, end indels, an empty read, one without a limit
    for (int m : {1, 63, 64, 65, 129, 257, 600, 1030}) {
        const std::string q = rand_seq(rng, m);
        const int k = m / 10 + 2;
        const uint32_t r0 = R.add(q, k);
        R.add(mutate(rng, q, 10), k);
        R.add(rand_seq(rng, 6) + mutate(rng, q, 5), k);
        R.add(mutate(rng, q, 5) + rand_seq(rng, 6), k);
        R.add(q.substr(std::min<size_t>(3, q.size())), k);
        R.add("", m);
        R.add(rand_seq(rng, m + 40), -1);
        R.add(rand_seq(rng, m + 70), k);                       // above the limit
        jobs.push_back(smx_cons_job{r0, r0, 8});
    }
    jobs.push_back(smx_cons_job{0, 3, 0});                     // no members
    ConsPlan P;
    std::string why;
    const uint32_t n_reads = (uint32_t)R.k.size();
    // what the plan must refuse
    {
        std::vector<smx_cons_job> bad = jobs;
        bad.push_back(smx_cons_job{5, 0, 1});                  // read 5 is empty: an empty draft
        if (cons_plan(R.bytes.data(), R.off.data(), n_reads, R.k.data(), bad.data(), (uint32_t)bad.size(), CONS_HIST_BYTES, &P, &why) != SMX_ERR_ARG)
            die("an empty draft was accepted");
        bad.back() = smx_cons_job{0, 6, 4};                    // overlaps the first two jobs
        if (cons_plan(R.bytes.data(), R.off.data(), n_reads, R.k.data(), bad.data(), (uint32_t)bad.size(), CONS_HIST_BYTES, &P, &why) != SMX_ERR_ARG)
            die("overlapping jobs were accepted");
        bad.back() = smx_cons_job{n_reads, 0, 0};
        if (cons_plan(R.bytes.data(), R.off.data(), n_reads, R.k.data(), bad.data(), (uint32_t)bad.size(), CONS_HIST_BYTES, &P, &why) != SMX_ERR_ARG)
            die("a draft out of range was accepted");
        bad.back() = smx_cons_job{0, n_reads - 1, 2};
        if (cons_plan(R.bytes.data(), R.off.data(), n_reads, R.k.data(), bad.data(), (uint32_t)bad.size(), CONS_HIST_BYTES, &P, &why) != SMX_ERR_ARG)
            die("members out of range were accepted");
        if (cons_plan(R.bytes.data(), R.off.data(), n_reads, R.k.data(), jobs.data(), (uint32_t)jobs.size(), 1024, &P, &why) != SMX_ERR_UNSUPPORTED)
            die("a history beyond its budget was accepted");
    }
    if (cons_plan(R.bytes.data(), R.off.data(), n_reads, R.k.data(), jobs.data(), (uint32_t)jobs.size(), CONS_HIST_BYTES, &P, &why) != SMX_OK)
        die(why.c_str());
    // buffers of exactly the planned sizes
    std::vector<uint32_t> rows(P.rows_words), votes(P.votes_words);
    std::vector<int32_t> dist(P.n_dist);
    std::vector<cons_pm> hpm(P.hist_slice * MINE_THREADS);
    std::vector<int> hs(P.hist_slice * MINE_THREADS);
    const size_t sw = (size_t)std::max(P.words_max0, 1) * MINE_THREADS;
    std::vector<u64> sP(sw), sM(sw);
    std::vector<int> sS(sw);
    std::vector<mine_u4> tbuf;
    size_t n_chunks = 0, at = 0;
    for (int c = 0; c < 6; c++) {
        n_chunks += P.chunks[c];
        if (P.n[c]) at += P.n[c] + 1;
    }
    if (at != P.chunk_start.size() || P.align.size() + 1 != jobs.size()) die("the class lists do not add up");
    long long aligned = 0, checksum = 0;
    for (const ConsJobDev &J : P.align) {
        const Query Q(R.bytes.data() + R.off[J.draft], P.len[J.draft]);
        for (uint32_t i = 0; i < J.n; i++) {
            const uint32_t r = J.r0 + i;
            const int n = P.len[r], lane = (int)((i * 37 + 127) % MINE_THREADS);
            tbuf.assign((size_t)n / 16 + 1, mine_u4{0, 0, 0, 0});
            memcpy(tbuf.data(), R.bytes.data() + R.off[r], (size_t)n);
            const unsigned char *t = reinterpret_cast<const unsigned char *>(tbuf.data());
            const int k = (R.k[J.draft] < 0 || R.k[r] < 0) ? -1 : std::max(R.k[J.draft], R.k[r]);
            const ConsHist H{hpm.data() + lane, hs.data() + lane, (int)J.B};
            uint32_t *row = rows.data() + J.rows_off + (size_t)i * (Q.m + 1);
            const int d = chunk_with_wr(CHUNK_CLASS_WORDS[chunk_class((size_t)Q.W)],
                                        [&](auto WR) { return pair_in_class<WR>(H, Q, k, t, n, row, sP, sM, sS, lane); });
            dist[J.dist_off + i] = d;
            if (d < 0) continue;
            aligned++;
            checksum += d;
            for (int p = 0; p <= Q.m; p++) {                   // the vote table of the job, as the vote kernel fills it
                uint32_t v[SMX_CONS_VOTE_WORDS] = {0};
                cons_vote_word(row[p], v);
                for (int x = 0; x < SMX_CONS_VOTE_WORDS; x++) votes[J.votes_off + (size_t)p * SMX_CONS_VOTE_WORDS + x] += v[x];
            }
        }
    }
    if (dist[0] != 0 || dist[5] != 1 || dist[7] != -1) die("unexpected distances in the first job");
    printf("jobs %zu chunks %zu aligned %lld checksum %lld\n", P.jobs.size(), n_chunks, aligned, checksum);
    return 0;
}
