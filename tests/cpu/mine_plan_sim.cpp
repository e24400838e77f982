// CPU simulation of a whole specimine call: the plan (specimux_amd/csrc/smx_mine_plan.h) and the kernel as a host loop
// over the planned chunks (mine_host.h), every distance and every best identity compared (==) with the full-matrix HW
// recurrence written here (mine_cases.h, mine_ref_hw).  The shapes are those of mine_cases.h, run with the production
// scratch budget and with a budget of one slice (one workgroup walks all chunks of the generic class).
// Built and run by tests/test_mine_plan_cpu.py (g++, no GPU).  Prints "<counter> <value>" lines and "<n> mismatches".
#include "mine_cases.h"

using namespace smx;

int main() {
    const MineCase C = mine_case(7);
    std::map<std::pair<uint32_t, uint32_t>, int> ref;
    for (const smx_mine_job &J : C.jobs)
        for (uint32_t qi = 0; qi < J.nq; qi++)
            for (uint32_t ti = 0; ti < J.nt; ti++) {
                const std::pair<uint32_t, uint32_t> key{J.q0 + qi, J.t0 + ti};
                if (!ref.count(key)) ref[key] = mine_ref_hw(C.query(key.first), C.target(key.second));
            }
    MineCaseTotals T;
    mine_case_run(C, 0, &ref, &T);
    mine_case_run(C, 1, &ref, &T);
    printf("ref_pairs %zu\n", ref.size());
    mine_case_print(T);
    return T.mismatches ? 1 : 0;
}
