// CPU simulation of a whole inner-scan call: the plan (specimux_amd/csrc/smx_inner_plan.h: pattern tables, launch groups
// under a budget, unit prefix, buffer sizes) and the two kernels as host loops over it (inner_host.h), every output
// compared (==) with the definition of a hit applied to the last row of the full HW recurrence over the whole read
// (inner_cases.h).  The shapes are those of inner_cases.h: Q = 1 .. 128, H = 1 and 8, margin = 0 and 80, reads around
// the piece boundaries and of 20 000 bases, three budgets, both entries; the results must not depend on the budget.
// Built and run by tests/test_inner_plan_cpu.py (g++, no GPU).  Prints "<counter> <value>" lines and "<n> mismatches".
#include "inner_cases.h"

using namespace smx;

int main() {
    InnerCaseTotals T;
    inner_cases_run(true, &T);
    inner_cases_print(T);
    return T.mismatches ? 1 : 0;
}
