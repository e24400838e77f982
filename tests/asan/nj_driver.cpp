// AddressSanitizer / UBSan driver for the host side of smx_nj: the plan of a call (smx_nj_plan.h: the argument checks, the
// buffer sizes, the launch counts) and the kernels' bodies as host loops (tests/cpu/nj_host.h over smx_nj_core.h), run the
// way smx_nj.hip indexes its buffers, over heap blocks of exactly the planned sizes, so that any index the plan did not
// budget for -- a matrix entry, a row sum, a row minimum, a merge record, an entry of the triangle -- is a heap overflow.
// n = 0 .. 5, 64, 65 and 257, random, all-equal and ladder matrices, the three visiting orders.  CPU only; built and run
// by tests/test_nj_asan.py with g++ -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../cpu/nj_host.h"

using namespace smx;

static void die(const char *what) { fprintf(stderr, "driver: %s\n", what); exit(2); }

int main() {
    std::mt19937 rng(5);
    NjCounters K;
    unsigned long long calls = 0, merges = 0, refusals = 0;
    for (uint32_t n : {0u, 1u, 2u, 3u, 4u, 5u, 64u, 65u, 257u})
        for (int kind = 0; kind < 3; kind++) {
            const size_t entries = (size_t)n * (n ? n - 1 : 0) / 2;
            int32_t *tri = new int32_t[entries];             // exactly the triangle: nothing behind it may be read
            size_t at = 0;
            for (uint32_t i = 0; i < n; i++)
                for (uint32_t j = i + 1; j < n; j++, at++)
                    tri[at] = kind == 0 ? 1 + (int32_t)(rng() % 3000) : kind == 1 ? 9 : 3 * (int32_t)j + 1 + (int32_t)((i + j) % 2);
            NjHostResult first;
            for (NjOrder order : {NJ_FORWARD, NJ_REVERSED, NJ_SHUFFLED}) {
                NjHostResult got;
                std::string why;
                if (nj_host_call(tri, n, order, 17u + n, &got, &K, &why) != SMX_OK) die(why.c_str());
                if (got.merges.size() != (n > 3 ? n - 3 : 0)) die("merge count");
                for (size_t t = 0; t < got.merges.size(); t++) {
                    const smx_nj_merge &m = got.merges[t];
                    if (m.n_active != n - t || m.a >= n + t || m.b >= n + t || m.a == m.b || m.pad != 0) die("merge record");
                }
                for (uint32_t i = 0; i < 3; i++)
                    if (got.last[i] >= (n > 3 ? 2 * n - 3 : n ? n : 1)) die("last node");
                if (order == NJ_FORWARD) first = got;
                else if (got.merges.size() != first.merges.size() ||
                         (first.merges.size() && memcmp(got.merges.data(), first.merges.data(), first.merges.size() * sizeof(smx_nj_merge))) ||
                         memcmp(got.last, first.last, sizeof got.last) || memcmp(got.last_d, first.last_d, sizeof got.last_d))
                    die("the visiting order changed the records");
                calls++;
                merges += got.merges.size();
            }
            // a negative entry anywhere is refused before anything is sized
            if (entries) {
                NjPlan P;
                std::string why;
                smx_nj_merge m = {};
                uint32_t last[3] = {0, 0, 0};
                double last_d[3] = {0, 0, 0};
                tri[entries - 1] = -1;
                if (nj_plan(tri, n, &m, last, last_d, &P, &why) != SMX_ERR_ARG) die("negative entry accepted");
                refusals++;
            }
            delete[] tri;
        }
    printf("calls %llu merges %llu iterations %llu moves %llu moves_none %llu ties %llu refusals %llu\n", calls, merges,
           (unsigned long long)K.iterations, (unsigned long long)K.moves, (unsigned long long)K.moves_none,
           (unsigned long long)K.ties, refusals);
    return 0;
}
