// AddressSanitizer / UBSan driver for the host side of the crosstalk calls: the plan of a call (smx_nearest_plan.h:
// argument checks, class lists, runs, chunk prefix, grids, scratch size) and the kernel as a host loop over the planned
// chunks (tests/cpu/nearest_host.h, which indexes every buffer by the kernel's own expressions), over buffers of exactly
// the planned sizes -- the padded sequences, the Peq table of the LDS request, the scratch slices, the keys and the
// distances -- so that any index the plan did not budget for is a heap overflow.  CPU only; built and run by
// tests/test_nearest_asan.py with g++ -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "nearest_host.h"

using namespace smx;

static void die(const char *what) { fprintf(stderr, "driver: %s\n", what); exit(2); }

struct Seqs {
    std::string bytes;
    std::vector<uint64_t> off{0};
    std::vector<int32_t> k;
    std::vector<uint32_t> group;
    uint32_t add(const std::string &s, int kk, uint32_t g) {
        bytes += s;
        off.push_back(bytes.size());
        k.push_back(kk);
        group.push_back(g);
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

int main() {
    std::mt19937 rng(7);
    Seqs R;
    // refs of every state class, two of them twice; then the reads of three jobs: copies, mutated copies, end indels, an
    // empty read, one without a limit, an unrelated one
    const int lens[] = {1, 63, 64, 65, 129, 257, 600, 1030, 1100};
    for (int m : lens) R.add(rand_seq(rng, m), m / 10 + 2, (uint32_t)R.k.size());
    R.add(R.bytes.substr(R.off[3], R.off[4] - R.off[3]), 8, 3);
    R.add(R.bytes.substr(R.off[7], R.off[8] - R.off[7]), 105, 500);
    const uint32_t nq = (uint32_t)R.k.size();
    std::vector<smx_nearest_job> jobs;
    for (int nt : {1, 130, 40}) {
        const uint32_t t0 = (uint32_t)R.k.size();
        for (int i = 0; i < nt; i++) {
            const uint32_t src = (uint32_t)(rng() % nq);
            const std::string q = R.bytes.substr(R.off[src], R.off[src + 1] - R.off[src]);
            const int kk = (int)q.size() / 10 + 2;
            switch (i % 6) {
                case 0: R.add(q, kk, R.group[src]); break;
                case 1: R.add(mutate(rng, q, 10), kk, R.group[src]); break;
                case 2: R.add(rand_seq(rng, 6) + mutate(rng, q, 5), kk, (uint32_t)(rng() % nq)); break;
                case 3: R.add("", (int)q.size(), R.group[src]); break;
                case 4: R.add(rand_seq(rng, (int)q.size() + 40), -1, 900); break;
                default: R.add(rand_seq(rng, (int)q.size() + 70), kk, R.group[src]); break;   // above the limit
            }
        }
        jobs.push_back(smx_nearest_job{0, nq, t0, (uint32_t)nt});
    }
    jobs.back().q0 = 2;                                            // the last job: a sub-range of the refs
    jobs.back().nq = nq - 4;
    jobs.push_back(smx_nearest_job{0, nq, 0, 0});                  // no reads
    jobs.push_back(smx_nearest_job{0, 0, 0, 3});                   // no refs (its reads are sequences 0..2)
    const uint32_t n_seqs = (uint32_t)R.k.size();
    NearestPlan P;
    std::string why;
    auto plan = [&](const std::vector<smx_nearest_job> &J) {
        return nearest_plan(R.bytes.data(), R.off.data(), n_seqs, J.data(), (uint32_t)J.size(), &P, &why);
    };
    {   // what the plan must refuse
        std::vector<smx_nearest_job> bad = jobs;
        uint32_t empty = 0;
        while (empty < n_seqs && R.off[empty + 1] != R.off[empty]) empty++;
        if (empty == n_seqs) die("no empty read to test with");
        bad.push_back(smx_nearest_job{empty, 1, n_seqs - 1, 0});
        if (plan(bad) != SMX_ERR_ARG) die("an empty ref was accepted");
        bad.back() = smx_nearest_job{n_seqs, 1, 0, 0};
        if (plan(bad) != SMX_ERR_ARG) die("a ref out of range was accepted");
        bad.back() = smx_nearest_job{0, 1, n_seqs - 1, 2};
        if (plan(bad) != SMX_ERR_ARG) die("reads out of range were accepted");
        bad.back() = smx_nearest_job{0, 1, jobs[1].t0 + 5, 2};
        if (plan(bad) != SMX_ERR_ARG) die("overlapping read ranges were accepted");
    }
    if (plan(jobs) != SMX_OK) die(why.c_str());
    const NearestHostSeqs S(R.bytes.data(), R.off.data(), n_seqs);
    long long found = 0, checksum = 0, chunks = 0, plans = 0;
    std::vector<u64> first_own, first_other;
    for (uint64_t G : {(uint64_t)1, (uint64_t)9, UINT64_MAX}) {
        nearest_plan_runs(&P, G);
        size_t at = 0, n_runs = 0;
        for (int c = 0; c < 6; c++) {
            n_runs += P.n[c];
            if (P.n[c]) at += P.n[c] + 1;
        }
        if (at != P.chunk_start.size() || n_runs != P.runs.size()) die("the class lists do not add up");
        // buffers of exactly the planned sizes
        std::vector<u64> own(P.n_best, NEAREST_NONE), other(P.n_best, NEAREST_NONE), scratch(P.scratch_words);
        std::vector<int32_t> dist(P.n_dist, -7);
        NearestHostCounts C;
        nearest_host_run(P, S, R.k.data(), R.group.data(), own.data(), other.data(), nullptr, scratch.data(), &C);
        nearest_host_run(P, S, R.k.data(), R.group.data(), nullptr, nullptr, dist.data(), scratch.data(), nullptr);
        for (int32_t d : dist) if (d == -7) die("a distance was not written");
        if (plans == 0) { first_own = own; first_other = other; }
        else if (own != first_own || other != first_other) die("the keys depend on the run length");
        chunks += C.chunks;
        plans++;
    }
    for (size_t i = 0; i < first_own.size(); i++)
        for (u64 key : {first_own[i], first_other[i]})
            if (key != NEAREST_NONE) { found++; checksum += (long long)(key >> 32); }
    // the first job's read is a copy of some ref: distance 0 to a ref of its own group
    if (first_own[0] >> 32 != 0) die("unexpected key of the first job's read");
    // the reads of the job without refs keep both keys
    for (size_t i = first_own.size() - 3; i < first_own.size(); i++)
        if (first_own[i] != NEAREST_NONE || first_other[i] != NEAREST_NONE) die("a key without a ref");
    printf("jobs %zu plans %lld chunks %lld reads %zu found %lld checksum %lld\n", P.jobs.size(), plans, chunks, first_own.size(),
           found, checksum);
    return 0;
}
