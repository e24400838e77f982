// AddressSanitizer / UBSan driver for the host side of the clusters calls: the plan of a call (smx_pairs_plan.h: argument
// checks, padded reads, jobs with offsets, rows by class, chunk prefix, grids, scratch size, the mirror of the triangle)
// and the kernel as a host loop over the planned chunks (tests/cpu/pairs_host.h, which indexes every buffer by the
// kernel's own expressions), over buffers of exactly the planned sizes -- the padded reads, the limits, the Peq table of
// the LDS request, the row list and prefix of each launch, the scratch slices, the packed triangles and the adjacency
// matrices -- so that any index the plan did not budget for is a heap overflow.  The shapes are those of the CPU
// simulation (tests/cpu/pairs_cases.h).  CPU only; built and run by tests/test_pairs_asan.py with
// g++ -fsanitize=address,undefined.
#include "pairs_cases.h"

using namespace smx;

static void die(const char *what) { fprintf(stderr, "driver: %s\n", what); exit(2); }

int main() {
    const PairsCase C = pairs_case(5);
    PairsPlan P;
    std::string why;
    auto plan = [&](bool distances, const std::vector<uint64_t> &off, const std::vector<smx_pairs_job> &J) {
        return pairs_plan(distances, C.bytes.data(), off.data(), C.n_reads(), J.data(), (uint32_t)J.size(), CHUNK_SCRATCH_BYTES, &P, &why);
    };
    {   // what the plan must refuse, as the calls do
        std::vector<smx_pairs_job> bad = C.jobs;
        bad.push_back(smx_pairs_job{C.jobs[2].r0 + 5, 3});
        if (plan(true, C.off, bad) != SMX_ERR_ARG || why.find("overlap") == std::string::npos) die("overlapping jobs were accepted");
        bad.back() = smx_pairs_job{C.jobs[4].r0 + C.jobs[4].n - 1, 1};
        if (plan(false, C.off, bad) != SMX_ERR_ARG) die("a job inside the last read of another was accepted");
        bad.back() = smx_pairs_job{C.n_reads() - 1, 2};
        if (plan(true, C.off, bad) != SMX_ERR_ARG || why.find("out of bounds") == std::string::npos) die("reads out of range were accepted");
        bad.back() = smx_pairs_job{0xfffffffeu, 3};
        if (plan(true, C.off, bad) != SMX_ERR_ARG) die("a read range that wraps was accepted");
        bad.back() = smx_pairs_job{C.jobs[2].r0 + 5, 0};         // an empty job inside another overlaps nothing
        if (plan(true, C.off, bad) != SMX_OK) die("an empty job was refused");
        std::vector<uint64_t> off = C.off;
        off[4] = off[3] - 1;
        if (plan(true, off, C.jobs) != SMX_ERR_ARG) die("offsets that go back were accepted");
        // only jobs of 0 and 1 reads: a zero word each in neighbours mode, nothing in distances mode, and no row
        const std::vector<smx_pairs_job> ones{smx_pairs_job{3, 1}, smx_pairs_job{9, 0}, smx_pairs_job{5, 1}};
        if (plan(false, C.off, ones) != SMX_OK || P.n_out != 2 || !P.rows.empty() || P.jobs[2].out_off != 1) die("jobs of one read: not a word each");
        if (plan(true, C.off, ones) != SMX_OK || P.n_out != 0 || !P.rows.empty()) die("jobs of one read have distances");
    }
    PairsCaseTotals T;
    pairs_case_run(C, 0, nullptr, &T);
    pairs_case_run(C, 1, nullptr, &T);
    pairs_case_print(T);
    return T.mismatches ? 1 : 0;
}
