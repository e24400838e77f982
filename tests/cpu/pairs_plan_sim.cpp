// CPU simulation of a whole clusters call: the plan (specimux_amd/csrc/smx_pairs_plan.h), the kernel as a host loop over
// the planned chunks (pairs_host.h) and the mirror of the adjacency triangle, every distance and every adjacency word
// compared (==) with the full-matrix NW recurrence written here (pairs_cases.h, pairs_ref_nw).  The shapes are those of
// pairs_cases.h, run with the production scratch budget and with a budget of one slice.
// Built and run by tests/test_pairs_plan_cpu.py (g++, no GPU).  Prints "<counter> <value>" lines and "<n> mismatches".
#include "pairs_cases.h"

using namespace smx;

int main() {
    const PairsCase C = pairs_case(5);
    std::map<std::pair<uint32_t, uint32_t>, int> ref;
    std::vector<std::string> reads;
    for (uint32_t r = 0; r < C.n_reads(); r++) reads.push_back(C.read(r));
    for (const smx_pairs_job &J : C.jobs)
        for (uint32_t i = 0; i < J.n; i++)
            for (uint32_t j = i + 1; j < J.n; j++) ref[{J.r0 + i, J.r0 + j}] = pairs_ref_nw(reads[J.r0 + i], reads[J.r0 + j]);
    {   // overlapping jobs are refused
        std::vector<smx_pairs_job> bad = C.jobs;
        bad.push_back(smx_pairs_job{C.jobs[2].r0 + 5, 3});
        PairsPlan P;
        std::string why;
        if (pairs_plan(true, C.bytes.data(), C.off.data(), C.n_reads(), bad.data(), (uint32_t)bad.size(), CHUNK_SCRATCH_BYTES, &P, &why) != SMX_ERR_ARG ||
            why.find("overlap") == std::string::npos) {
            fprintf(stderr, "overlapping jobs were accepted\n");
            return 1;
        }
        printf("refused_overlap 1\n");
    }
    PairsCaseTotals T;
    pairs_case_run(C, 0, &ref, &T);
    pairs_case_run(C, 1, &ref, &T);
    printf("ref_pairs %zu\n", ref.size());
    pairs_case_print(T);
    return T.mismatches ? 1 : 0;
}
