// What the host twins of the chunked kernels share (mine_host.h, pairs_host.h, nearest_host.h, hits_host.h; the
// consensus simulation and driver take the dispatch): the walk over a call's launch table (ChunkLaunches,
// smx_chunk_plan.h) the way the launches and chunk_walk (smx_mine_lds.h) make it -- class after class, workgroup after
// workgroup over its chunks [b * per_block, (b + 1) * per_block), the first record found by chunk_owner's 64-lane search
// and checked against std::upper_bound, the owner advanced chunk by chunk -- and the one dispatch from a launch's
// run-time wr to the <WR> instantiation.  What a twin does inside a chunk stays in the twin.
#ifndef SMX_TESTS_CHUNK_WALK_HOST_H
#define SMX_TESTS_CHUNK_WALK_HOST_H
#include <type_traits>
#include <vector>

#include "chunk_owner_host.h"
#include "smx_chunk_plan.h"

namespace smx {

// f(std::integral_constant<int, WR>) for the WR of a launch: 1, 2, 4, 8, 16 words of state in registers, else 0 (scratch)
template <typename F> inline auto chunk_with_wr(int wr, F &&f) {
    switch (wr) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        default: return f(std::integral_constant<int, 0>{});
    }
}

struct ChunkWalkCounts {   // summed over the walks a twin makes; every *HostCounts starts with them
    long long chunks = 0, blocks = 0, records = 0;
    long long records_two_chunks = 0;   // records that own more than one chunk
    long long blocks_inside = 0;        // workgroups whose first chunk is not the first of its record
    long long owner_rounds_max = 0;
    long long class_blocks[CHUNK_CLASSES] = {0, 0, 0, 0, 0, 0};
};

struct ChunkStep {         // one chunk of the walk
    int c, wr;             // the class and the wr of its launch
    uint64_t block;        // the workgroup: blockIdx.x
    bool first;            // its first chunk: what a workgroup keeps from chunk to chunk starts afresh
    uint32_t p;            // the record of the class that owns the chunk, rec_at + p in the call's record list
    size_t rec_at;
    uint64_t v, at;        // the chunk among the class's, and among the record's: v - chunk_start[p]
};

// on_chunk(ChunkStep) for every chunk of every launch.  Each class's prefix is walked in a heap allocation of exactly
// n + 1 entries, so a caller under a sanitizer finds a search or an advance that leaves it.
template <typename F> inline void chunk_walk_host(const ChunkLaunches &L, ChunkWalkCounts *counts, F &&on_chunk) {
    chunk_for_each_class(L, [&](const ChunkLaunch &K) {
        const std::vector<uint64_t> chunk_start(L.chunk_start.begin() + K.start_at, L.chunk_start.begin() + K.start_at + K.n + 1);
        const uint64_t n_chunks = chunk_start[K.n], grid = (uint64_t)K.grid;
        if (n_chunks != L.chunks[K.c] || grid * K.per_block < n_chunks) host_twin_fail("the grid does not cover the class's chunks");
        for (uint32_t p = 0; p < K.n; p++) {
            if (chunk_start[p + 1] <= chunk_start[p]) host_twin_fail("a record without chunks");
            if (counts) counts->records_two_chunks += chunk_start[p + 1] - chunk_start[p] > 1;
        }
        if (counts) counts->records += K.n;
        for (uint64_t block = 0; block < grid; block++) {
            // chunk_span
            const uint64_t lo = block * K.per_block, hi = lo + K.per_block < n_chunks ? lo + K.per_block : n_chunks;
            if (lo >= n_chunks) host_twin_fail("a workgroup without chunks");
            int rounds = 0;
            uint32_t p = chunk_owner_host(chunk_start.data(), K.n, lo, &rounds);
            if (counts) {
                counts->blocks++;
                counts->class_blocks[K.c]++;
                counts->blocks_inside += chunk_start[p] < lo;
                counts->owner_rounds_max = std::max<long long>(counts->owner_rounds_max, rounds);
            }
            for (uint64_t v = lo; v < hi; v++) {
                while (chunk_start[p + 1] <= v) p++;
                if (counts) counts->chunks++;
                on_chunk(ChunkStep{K.c, K.wr, block, v == lo, p, K.rec_at, v, v - chunk_start[p]});
            }
        }
        return 0;
    });
}

}  // namespace smx

#endif  // SMX_TESTS_CHUNK_WALK_HOST_H
