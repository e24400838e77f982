// chunk_owner (specimux_amd/csrc/smx_mine_lds.h) over 64 emulated lanes: the same chunk_owner_step / _probe / _advance
// / _left (smx_mine_core.h) the device function runs, with the wave's ballot built lane by lane. The host twins of the
// chunked kernels (through chunk_walk_host.h; reach_host.h directly) find a workgroup's first record with it and check
// it against std::upper_bound; a probe outside the prefix's n + 1 entries is then an overflow of the buffer the caller
// handed in.
#ifndef SMX_TESTS_CHUNK_OWNER_HOST_H
#define SMX_TESTS_CHUNK_OWNER_HOST_H
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "smx_mine_core.h"

namespace smx {

[[noreturn]] inline void host_twin_fail(const char *what) {
    fprintf(stderr, "host twin: %s\n", what);
    exit(3);
}

// The last p with chunk_start[p] <= lo among n records (chunk_start has n + 1 entries, lo < chunk_start[n]).
// *rounds, if given, receives the rounds of the search.
inline uint32_t chunk_owner_host(const uint64_t *chunk_start, uint32_t n, uint64_t lo, int *rounds = nullptr) {
    const uint32_t n_records = n;
    uint32_t p = 0;
    int r = 0;
    while (n > 1) {
        const uint32_t step = chunk_owner_step(n);
        uint64_t ballot = 0;
        for (unsigned lane = 0; lane < 64; lane++) {
            const uint32_t idx = chunk_owner_probe(p, step, lane);
            const bool le = idx < p + n && chunk_start[idx] <= lo;
            if (le) ballot |= 1ull << lane;
        }
        if (!(ballot & 1) || (ballot & (ballot + 1))) host_twin_fail("chunk_owner: the lanes that hold are not a prefix with lane 0");
        const uint32_t count = (uint32_t)__builtin_popcountll(ballot);
        const uint32_t end = p + n;
        p += chunk_owner_advance(step, count);
        n = chunk_owner_left(step, end, p);
        r++;
    }
    if (rounds) *rounds = r;
    const uint32_t want = (uint32_t)(std::upper_bound(chunk_start, chunk_start + n_records, lo) - chunk_start) - 1;
    if (p != want) host_twin_fail("chunk_owner: the 64-way search and std::upper_bound disagree");
    return p;
}

// The search over prefixes of n records of 1..3 chunks each, for the first chunk of every `stride`-th workgroup of 8 and
// for the last chunk: n at and around the round thresholds 64, 4096 and 262 144.  Returns the most rounds a search took
// (4 from 262 145 records on); the prefix is an allocation of exactly n + 1 entries.
inline int chunk_owner_sweep(long long *searches) {
    int most = 0;
    for (uint32_t n : {1u, 2u, 63u, 64u, 65u, 4095u, 4096u, 4097u, 262143u, 262144u, 262145u, 300001u}) {
        std::vector<uint64_t> prefix((size_t)n + 1, 0);
        uint32_t x = n * 2654435761u + 1;
        for (uint32_t p = 0; p < n; p++) {
            x = x * 1664525u + 1013904223u;
            prefix[p + 1] = prefix[p] + 1 + (x >> 24) % 3;
        }
        const uint64_t n_chunks = prefix[n], stride = n > 5000 ? 97 : 1;
        for (uint64_t lo = 0; lo < n_chunks; lo += 8 * stride) {
            int rounds = 0;
            chunk_owner_host(prefix.data(), n, lo, &rounds);
            most = std::max(most, rounds);
            ++*searches;
        }
        int rounds = 0;
        if (chunk_owner_host(prefix.data(), n, n_chunks - 1, &rounds) != n - 1) host_twin_fail("chunk_owner: the last chunk is not the last record's");
        most = std::max(most, rounds);
        ++*searches;
    }
    return most;
}

}  // namespace smx

#endif  // SMX_TESTS_CHUNK_OWNER_HOST_H
