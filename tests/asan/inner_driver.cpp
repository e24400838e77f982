// AddressSanitizer / UBSan driver for the host side of the inner-scan calls: the plan of a call (smx_inner_plan.h: pattern
// checks, lead / PL / RW, the table blob, the launch groups under a budget with their unit prefix and buffer sizes) and
// the two kernels as host loops over it (tests/cpu/inner_host.h, which indexes every buffer by the kernels' own
// expressions), over buffers of exactly the planned sizes -- the code map, the match words and pm / pk / jmap of each
// class, the bases up to the 16-byte word that holds the group's last byte, roff / ustart / unit_read, the records and
// the he | hd | nh output -- so that any index the plan did not budget for is a heap overflow.  The shapes are those of
// the CPU simulation (tests/cpu/inner_cases.h).  CPU only; built and run by tests/test_inner_asan.py with
// g++ -fsanitize=address,undefined.
#include "inner_cases.h"

using namespace smx;

static void die(const char *what) { fprintf(stderr, "driver: %s\n", what); exit(2); }

int main() {
    {   // what the plan must refuse, as the calls do
        InnerPlan P;
        std::string why;
        auto plan = [&](const std::string &pats, const std::vector<uint32_t> &poff, const std::vector<int32_t> &k, uint32_t Q, int32_t margin, uint32_t H) {
            return inner_plan(pats.data(), poff.data(), Q, k.data(), margin, H, 0, INNER_DEFAULT_BUDGET, inner_host_alphabet(), &P, &why);
        };
        const std::string two = "ACGTNACGTRY";
        const std::vector<uint32_t> poff{0, 5, 11};
        const std::vector<int32_t> k{1, 2};
        if (plan(two, poff, k, 2, 10, 3) != SMX_OK || P.lead != 8 || P.PL != 64 || P.RW != 5) die("a good call was refused, or lead / PL / RW are off");
        if (plan(two, poff, k, 0, 10, 3) != SMX_ERR_ARG) die("no patterns were accepted");
        std::vector<uint32_t> many(INNER_MAX_PATTERNS + 2, 0);
        if (plan(two, many, std::vector<int32_t>(INNER_MAX_PATTERNS + 1, 0), INNER_MAX_PATTERNS + 1, 10, 3) != SMX_ERR_ARG) die("129 patterns were accepted");
        if (plan(two, poff, k, 2, 10, 0) != SMX_ERR_ARG || plan(two, poff, k, 2, 10, INNER_MAX_HITS + 1) != SMX_ERR_ARG) die("a bad max_hits was accepted");
        if (plan(two, poff, k, 2, -1, 3) != SMX_ERR_ARG) die("a negative margin was accepted");
        if (plan(two, {0, 5, 5}, k, 2, 10, 3) != SMX_ERR_ARG || why != "pattern 1: length outside 1..64") die("an empty pattern was accepted");
        if (plan(std::string(70, 'A'), {0, 5, 70}, k, 2, 10, 3) != SMX_ERR_ARG) die("a pattern of 65 letters was accepted");
        if (plan(two, poff, {1, 6}, 2, 10, 3) != SMX_ERR_ARG || why != "pattern 1: threshold 6 outside 0..5") die("a threshold of m was accepted");
        if (plan(two, poff, {-1, 2}, 2, 10, 3) != SMX_ERR_ARG) die("a negative threshold was accepted");
        if (plan("ACGTNACGTRy", poff, k, 2, 10, 3) != SMX_ERR_ARG || why.find("outside the IUPAC DNA alphabet") == std::string::npos) die("a lower-case pattern letter was accepted");
        if (plan(two, poff, k, 2, 10, 3) != SMX_OK) die("a good call was refused");
        const uint32_t len[2] = {100, 0x80000000u};
        InnerGroup g;
        if (P.next_group(len, 2, 0, &g, &why) != SMX_ERR_ARG || why != "read 1: longer than 2^31 - 1 bases") die("a read of 2^31 bases was accepted");
    }
    InnerCaseTotals T;
    inner_cases_run(false, &T);
    inner_cases_print(T);
    return T.mismatches ? 1 : 0;
}
