// AddressSanitizer / UBSan driver for the host side of the identify calls: the plan of a call (smx_hits_plan.h: argument
// checks, orders, windows, records by class, chunk prefix, grids, scratch size) and the kernel as a host loop over the
// planned chunks (tests/cpu/hits_host.h, which indexes every buffer by the kernel's own expressions), over buffers of
// exactly the planned sizes -- the padded sequences, the Peq table of the LDS request, the scratch slices, the keys and
// the distances -- so that any index the plan did not budget for is a heap overflow.  CPU only; built and run by
// tests/test_hits_asan.py with g++ -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "hits_host.h"

using namespace smx;

static void die(const char *what) { fprintf(stderr, "driver: %s\n", what); exit(2); }

struct Seqs {
    std::string bytes;
    std::vector<uint64_t> off{0};
    std::vector<int32_t> k;
    uint32_t add(const std::string &s, int kk) {
        bytes += s;
        off.push_back(bytes.size());
        k.push_back(kk);
        return (uint32_t)k.size() - 1;
    }
    std::string get(uint32_t i) const { return bytes.substr(off[i], off[i + 1] - off[i]); }
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
    return out.empty() ? s : out;
}

int main() {
    std::mt19937 rng(11);
    Seqs R;
    // queries of every state class; then the targets of three jobs: flanked, trimmed and mutated copies, twins, strangers
    const int lens[] = {1, 63, 64, 65, 129, 257, 600, 1030, 1100};
    for (int m : lens) R.add(rand_seq(rng, m), m / 10 + 2);
    const uint32_t nq = (uint32_t)R.k.size();
    std::vector<smx_hits_job> jobs;
    const int nts[] = {1, 300, 40};
    uint32_t q_at = 0;
    const uint32_t q_per_job[] = {2, 4, 3};
    uint32_t shared_t0 = 0;
    for (int j = 0; j < 3; j++) {
        const uint32_t t0 = (uint32_t)R.k.size();
        if (j == 1) shared_t0 = t0;
        for (int i = 0; i < nts[j]; i++) {
            const uint32_t src = q_at + (uint32_t)(rng() % q_per_job[j]);
            const std::string q = R.get(src);
            const int kk = (int)q.size() / 10 + 2;
            switch (i % 6) {
                case 0: R.add(rand_seq(rng, 30) + q + rand_seq(rng, 30), kk); break;
                case 1: R.add(mutate(rng, q, 10), kk); break;
                case 2: R.add(q.substr(q.size() / 5, std::max<size_t>(1, q.size() / 2)), kk); break;
                case 3: R.add(q, -1); break;
                case 4: R.add(rand_seq(rng, (int)q.size() + 40), -1); break;
                default: R.add(rand_seq(rng, std::max(1, (int)q.size() - 7)), kk); break;
            }
        }
        jobs.push_back(smx_hits_job{q_at, q_per_job[j], t0, (uint32_t)nts[j]});
        q_at += q_per_job[j];
    }
    if (q_at != nq) die("the jobs do not use every query");
    const uint32_t extra = R.add(rand_seq(rng, 90), -1);               // a query of its own over the second job's targets
    jobs.push_back(smx_hits_job{extra, 1, shared_t0, 300});
    jobs.push_back(smx_hits_job{0, 0, shared_t0, 7});                  // no queries
    const uint32_t lone = R.add(rand_seq(rng, 20), 2);
    jobs.push_back(smx_hits_job{lone, 1, 0, 0});                       // no targets: its row stays empty
    R.add("", 0);                                                      // an empty sequence no job names
    const uint32_t n_seqs = (uint32_t)R.k.size();
    HitsPlan P;
    std::string why;
    auto plan = [&](const std::vector<smx_hits_job> &J, uint32_t K, uint32_t cov) {
        return hits_plan(R.bytes.data(), R.off.data(), n_seqs, J.data(), (uint32_t)J.size(), K, cov, &P, &why);
    };
    {   // what the plan must refuse
        std::vector<smx_hits_job> bad = jobs;
        bad.push_back(smx_hits_job{n_seqs - 1, 1, 0, 0});
        if (plan(bad, 5, 500) != SMX_ERR_ARG) die("an empty query was accepted");
        bad.back() = smx_hits_job{0, 0, n_seqs - 1, 1};
        if (plan(bad, 5, 500) != SMX_ERR_ARG) die("an empty target was accepted");
        bad.back() = smx_hits_job{n_seqs, 1, 0, 0};
        if (plan(bad, 5, 500) != SMX_ERR_ARG) die("a query out of range was accepted");
        bad.back() = smx_hits_job{lone, 0, n_seqs - 1, 2};
        if (plan(bad, 5, 500) != SMX_ERR_ARG) die("targets out of range were accepted");
        bad.back() = smx_hits_job{1, 2, shared_t0, 2};
        if (plan(bad, 5, 500) != SMX_ERR_ARG) die("overlapping query ranges were accepted");
        if (plan(jobs, 0, 500) != SMX_ERR_ARG || plan(jobs, 17, 500) != SMX_ERR_ARG) die("a bad K was accepted");
        if (plan(jobs, 5, 1001) != SMX_ERR_ARG) die("a bad coverage was accepted");
    }
    const NearestHostSeqs S(R.bytes.data(), R.off.data(), n_seqs);
    long long found = 0, checksum = 0, chunks = 0, plans = 0, pairs = 0;
    for (uint32_t cov : {0u, 500u, 1000u})
        for (int K : {1, 5, 16}) {
            if (plan(jobs, (uint32_t)K, cov) != SMX_OK) die(why.c_str());
            size_t at = 0, n_recs = 0;
            for (int c = 0; c < 6; c++) {
                n_recs += P.n[c];
                if (P.n[c]) at += P.n[c] + 1;
            }
            if (at != P.chunk_start.size() || n_recs != P.recs.size()) die("the class lists do not add up");
            // buffers of exactly the planned sizes
            std::vector<u64> keys(P.n_rows * K, HITS_NONE), scratch(P.scratch_words);
            std::vector<int32_t> dist(P.n_dist, -1);
            HitsHostCounts C;
            hits_host_run(P, S, R.k.data(), K, keys.data(), nullptr, scratch.data(), &C);
            hits_host_run(P, S, R.k.data(), K, nullptr, dist.data(), scratch.data(), nullptr);
            if ((uint64_t)C.pairs != P.n_pairs) die("the loop and the plan disagree about the pairs");
            // the keys against the distances: per query the K smallest, ascending, padded
            for (size_t j = 0; j < jobs.size(); j++)
                for (uint32_t q = 0; q < jobs[j].nq; q++) {
                    const u64 *row = keys.data() + (P.jobs[j].row_off + q) * K;
                    long long hits = 0;
                    for (uint32_t t = 0; t < jobs[j].nt; t++) hits += dist[P.jobs[j].dist_off + (uint64_t)q * jobs[j].nt + t] >= 0;
                    for (int s = 0; s < K; s++) {
                        if ((s < hits) != (row[s] != HITS_NONE)) die("a row does not hold min(K, hits) keys");
                        if (s && row[s] != HITS_NONE && row[s] <= row[s - 1]) die("a row is not ascending");
                        if (row[s] == HITS_NONE) continue;
                        const uint32_t t = hits_key_target(row[s]);
                        if (t >= jobs[j].nt) die("a key names a target outside its job");
                        if (dist[P.jobs[j].dist_off + (uint64_t)q * jobs[j].nt + t] != (int32_t)hits_key_d(row[s])) die("a key's distance is not the pair's");
                        found++;
                        checksum += (long long)hits_key_d(row[s]) + hits_key_ppm(row[s]) % 7;
                    }
                }
            chunks += C.chunks;
            pairs += C.pairs;
            plans++;
        }
    printf("jobs %zu plans %lld chunks %lld pairs %lld found %lld checksum %lld\n", jobs.size(), plans, chunks, pairs, found, checksum);
    return 0;
}
