// AddressSanitizer / UBSan driver for the host side of the bimera calls: the plan of a call (smx_reach_plan.h: argument
// checks, jobs, records, chunk prefix, grid, the forward and reversed padded sequences) and the kernel as a host loop
// over the planned chunks (tests/cpu/reach_host.h, which indexes every buffer by the kernel's own expressions), over
// buffers of exactly the planned sizes -- the padded sequences, the keys and the matrix -- so that any index the plan
// did not budget for, and any byte a slide reads behind the slack, is a heap overflow.  CPU only; built and run by
// tests/test_reach_asan.py with g++ -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "reach_host.h"

using namespace smx;

static void die(const char *what) { fprintf(stderr, "driver: %s\n", what); exit(2); }

struct Seqs {
    std::string bytes;
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> weight, need;
    uint32_t add(const std::string &s, uint32_t w, uint32_t nd) {
        bytes += s;
        off.push_back(bytes.size());
        weight.push_back(w);
        need.push_back(nd);
        return (uint32_t)weight.size() - 1;
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
    return out.empty() ? s : out;
}

int main() {
    std::mt19937 rng(19);
    Seqs R;
    std::vector<smx_reach_job> jobs;
    // three jobs of queries against relatives of every length around the 8- and 16-byte edges; the LAST sequence of the
    // call is one whose slide runs to its very end, so that the bytes read behind it are the slack itself
    const int lens[] = {1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130};
    const std::string root = rand_seq(rng, 130);
    const int nts[] = {1, 65, 140};
    uint32_t shared_t0 = 0;
    for (int j = 0; j < 3; j++) {
        const uint32_t q0 = (uint32_t)R.weight.size();
        for (int i = 0; i < 3; i++) R.add(mutate(rng, root.substr(0, lens[(j * 3 + i) % 14]), 20 * i), 1, (uint32_t)i);
        const uint32_t t0 = (uint32_t)R.weight.size();
        if (j == 1) shared_t0 = t0;
        for (int i = 0; i < nts[j]; i++) {
            const int L = lens[i % 14];
            switch (i % 4) {
                case 0: R.add(root.substr(0, L), (uint32_t)(i % 3), 0); break;
                case 1: R.add(root.substr(130 - L), 2, 0); break;
                case 2: R.add(mutate(rng, root.substr(0, L), 30), (uint32_t)(i % 3), 0); break;
                default: R.add(rand_seq(rng, L), 1, 0); break;
            }
        }
        jobs.push_back(smx_reach_job{q0, 3, t0, (uint32_t)nts[j]});
    }
    const uint32_t extra = R.add(root, 0, 0);                           // a query of its own over the second job's targets
    jobs.push_back(smx_reach_job{extra, 1, shared_t0, 65});
    jobs.push_back(smx_reach_job{0, 0, shared_t0, 7});                  // no queries
    const uint32_t lone = R.add(rand_seq(rng, 20), 1, 0);
    jobs.push_back(smx_reach_job{lone, 1, 0, 0});                       // no targets: its rows stay empty
    R.add("", 0, 0);                                                    // an empty sequence no job names
    const uint32_t tail = R.add(root.substr(0, 64), 5, 0);              // queries that are their own targets, at the very end
    R.add(root.substr(0, 64), 5, 0);
    jobs.push_back(smx_reach_job{tail, 2, tail, 2});
    const uint32_t n_seqs = (uint32_t)R.weight.size();
    ReachPlan P;
    std::string why;
    auto plan = [&](const std::vector<smx_reach_job> &J, uint32_t E) {
        return reach_plan(R.off.data(), n_seqs, J.data(), (uint32_t)J.size(), E, &P, &why);
    };
    {   // what the plan must refuse
        std::vector<smx_reach_job> bad = jobs;
        bad.push_back(smx_reach_job{tail - 1, 1, 0, 0});
        if (plan(bad, 5) != SMX_ERR_ARG) die("an empty query was accepted");
        bad.back() = smx_reach_job{0, 0, tail - 1, 1};
        if (plan(bad, 5) != SMX_ERR_ARG) die("an empty target was accepted");
        bad.back() = smx_reach_job{n_seqs, 1, 0, 0};
        if (plan(bad, 5) != SMX_ERR_ARG) die("a query out of range was accepted");
        bad.back() = smx_reach_job{0, 0, n_seqs - 1, 2};
        if (plan(bad, 5) != SMX_ERR_ARG) die("targets out of range were accepted");
        bad.back() = smx_reach_job{1, 2, shared_t0, 2};
        if (plan(bad, 5) != SMX_ERR_ARG) die("overlapping query ranges were accepted");
        if (plan(jobs, 16) != SMX_ERR_ARG) die("a bad E was accepted");
    }
    const ReachHostSeqs S(R.bytes.data(), R.off.data(), n_seqs);
    if (S.rc != SMX_OK) die(S.why.c_str());
    long long found = 0, checksum = 0, chunks = 0, plans = 0, items = 0;
    for (int E : {0, 1, 7, 15}) {
        if (plan(jobs, (uint32_t)E) != SMX_OK) die(why.c_str());
        if (P.chunk_start.size() != P.recs.size() + 1 || P.grid * P.per_block < P.chunks) die("the chunk list does not add up");
        // buffers of exactly the planned sizes
        std::vector<u64> keys(P.n_keys, HITS_NONE);
        std::vector<uint32_t> values(P.n_values, REACH_NOT_ELIGIBLE);
        ReachHostCounts C;
        reach_host_run(P, S, n_seqs, R.weight.data(), R.need.data(), E, keys.data(), nullptr, &C);
        reach_host_run(P, S, n_seqs, R.weight.data(), R.need.data(), E, nullptr, values.data(), nullptr);
        // the keys against the matrix: per (query, side, e) the two furthest eligible targets, ascending keys, padded
        for (size_t j = 0; j < jobs.size(); j++)
            for (uint32_t q = 0; q < jobs[j].nq; q++)
                for (int side = 0; side < 2; side++)
                    for (int e = 0; e <= E; e++) {
                        const u64 *slots = keys.data() + reach_slot_at(P.jobs[j].row_off + q, side, e, E);
                        long long eligible = 0;
                        uint32_t furthest = 0;
                        for (uint32_t t = 0; t < jobs[j].nt; t++) {
                            const uint32_t v = values[reach_value_at(P.jobs[j].mat_off + (uint64_t)q * jobs[j].nt + t, side, e, E)];
                            if (v == REACH_NOT_ELIGIBLE) continue;
                            eligible++;
                            furthest = std::max(furthest, v);
                            if (e && v < values[reach_value_at(P.jobs[j].mat_off + (uint64_t)q * jobs[j].nt + t, side, e - 1, E)]) die("reach falls with e");
                        }
                        for (int s = 0; s < REACH_SLOTS; s++) {
                            if ((s < eligible) != (slots[s] != HITS_NONE)) die("a slot pair does not hold min(2, eligible) keys");
                            if (s && slots[s] != HITS_NONE && slots[s] <= slots[s - 1]) die("a slot pair is not ascending");
                            if (slots[s] == HITS_NONE) continue;
                            const uint32_t t = reach_key_target(slots[s]);
                            if (t < jobs[j].t0 || t >= jobs[j].t0 + jobs[j].nt) die("a key names a target outside its job");
                            if (values[reach_value_at(P.jobs[j].mat_off + (uint64_t)q * jobs[j].nt + (t - jobs[j].t0), side, e, E)] != reach_key_reach(slots[s])) die("a key's reach is not the pair's");
                            if (s == 0 && reach_key_reach(slots[s]) != furthest) die("the first key is not the furthest reach");
                            found++;
                            checksum += reach_key_reach(slots[s]) % 11 + 1;
                        }
                    }
        chunks += C.chunks;
        items += C.items;
        plans++;
    }
    printf("jobs %zu plans %lld chunks %lld items %lld found %lld checksum %lld\n", jobs.size(), plans, chunks, items, found, checksum);
    return 0;
}
