// AddressSanitizer / UBSan driver for the host side of smx_flank_assign: the plan of a call (smx_flank_plan.h: argument
// checks, the candidates regrouped by primer with their match words) over arguments that are heap allocations of exactly
// the sizes the call names (tests/cpu/flank_plan_host.h, which also checks the plan against a plain stable sort), so that
// any byte read behind the keys, the text, the offsets or the primers, and any slot written outside the planned vectors,
// is a report.  CPU only; built and run by tests/test_flank_asan.py with g++ -fsanitize=address,undefined.
#include "flank_plan_host.h"

int main() {
    smx::FlankPlanCounts C;
    smx::flank_plan_cases(&C);
    smx::flank_plan_print(C);
    printf("%ld mismatches\n", C.mismatches);
    return C.mismatches ? 1 : 0;
}
