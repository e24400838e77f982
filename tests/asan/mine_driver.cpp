// AddressSanitizer / UBSan driver for the host side of the specimine calls: the plan of a call (smx_mine_plan.h: argument
// checks, padded targets, jobs with offsets, records by class, chunk prefix, grids, scratch size) and the kernel as a host
// loop over the planned chunks (tests/cpu/mine_host.h, which indexes every buffer by the kernel's own expressions), over
// buffers of exactly the planned sizes -- the queries, the padded targets, the Peq table of the LDS request, the record
// list and prefix of each launch, the scratch slices, the distances and the best identities -- so that any index the
// plan did not budget for is a heap overflow.  The shapes are those of the CPU simulation (tests/cpu/mine_cases.h).
// CPU only; built and run by tests/test_mine_asan.py with g++ -fsanitize=address,undefined.
#include "mine_cases.h"

using namespace smx;

static void die(const char *what) { fprintf(stderr, "driver: %s\n", what); exit(2); }

int main() {
    const MineCase C = mine_case(7);
    const std::vector<int32_t> k = mine_case_k(C, 0);
    MinePlan P;
    std::string why;
    auto plan = [&](const std::vector<uint64_t> &qoff, const std::vector<uint64_t> &toff, const std::vector<smx_mine_job> &J) {
        return mine_plan(C.qbytes.data(), qoff.data(), C.nq(), k.data(), C.tbytes.data(), toff.data(), C.nt(), J.data(),
                         (uint32_t)J.size(), CHUNK_SCRATCH_BYTES, &P, &why);
    };
    {   // what the plan must refuse, as the calls do
        std::vector<smx_mine_job> bad = C.jobs;
        bad.push_back(smx_mine_job{C.nq(), 1, 0, 0, 0.0});
        if (plan(C.qoff, C.toff, bad) != SMX_ERR_ARG || why.find("out of bounds") == std::string::npos) die("a query out of range was accepted");
        bad.back() = smx_mine_job{0, 1, C.nt() - 1, 2, 0.0};
        if (plan(C.qoff, C.toff, bad) != SMX_ERR_ARG) die("targets out of range were accepted");
        bad.back() = smx_mine_job{0xffffffffu, 2, 0, 0, 0.0};
        if (plan(C.qoff, C.toff, bad) != SMX_ERR_ARG) die("a query range that wraps was accepted");
        std::vector<uint64_t> qoff = C.qoff;
        qoff[3] = qoff[2];
        if (plan(qoff, C.toff, C.jobs) != SMX_ERR_ARG || why != "query 2 is empty") die("an empty query was accepted");
        qoff[3] = qoff[2] - 1;
        if (plan(qoff, C.toff, C.jobs) != SMX_ERR_ARG) die("query offsets that go back were accepted");
        std::vector<uint64_t> toff = C.toff;
        toff[5] = toff[4] - 1;
        if (plan(C.qoff, toff, C.jobs) != SMX_ERR_ARG || why != "target 4: bad offsets") die("target offsets that go back were accepted");
        // a query whose table does not fit the LDS: 256 distinct bytes x 81 words
        std::string wide(5120, 'A');
        for (size_t i = 0; i < wide.size(); i++) wide[i] = (char)(i % 256);
        const std::vector<uint64_t> woff{0, wide.size()};
        const int32_t wk = -1;
        const smx_mine_job wj{0, 1, 0, 1, 0.0};
        if (mine_plan(wide.data(), woff.data(), 1, &wk, C.tbytes.data(), C.toff.data(), C.nt(), &wj, 1, CHUNK_SCRATCH_BYTES, &P, &why) !=
                SMX_ERR_UNSUPPORTED || why.find("do not fit the LDS") == std::string::npos)
            die("a query too wide for the LDS was accepted");
        if (plan(C.qoff, C.toff, {}) != SMX_OK || P.n_dist || P.n_best || !P.pairs.empty()) die("a call without jobs is not empty");
    }
    MineCaseTotals T;
    mine_case_run(C, 0, nullptr, &T);
    mine_case_run(C, 1, nullptr, &T);
    mine_case_print(T);
    return T.mismatches ? 1 : 0;
}
