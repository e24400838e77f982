// CPU simulation of the statistics kernel (specimux_amd/csrc/smx_stats.hip): the same per-read code
// (smx_stats_core.h: candidate enumeration, scoring, key packing, table insert) over hit tables and primary records
// read from a file, in the kernel's shape -- workgroup chunks of reads counted into a small local table that is
// flushed into the global one.  No GPU needed.
//
//   stats_sim INPUT CAPACITY [GRID]
// INPUT (little endian): int32 NP, NPAIR, preorient, n_reads; int32 pdir[NP], pair_f[NPAIR], pair_r[NPAIR];
// smx_hit hits[n_reads][2 * NP]; smx_op ops[n_reads].
// Prints "counters ..." (coverage of the input), "fallback I" per read left to the host and "key HEX COUNT" per row;
// exits 4 with "SMX_ERR_OVERFLOW ..." when an increment finds the global table full.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "smx_stats_core.h"

using namespace smx;

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: stats_sim INPUT CAPACITY [GRID]\n"); return 2; }
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) { perror(argv[1]); return 2; }
    int32_t head[4];
    if (fread(head, 4, 4, fh) != 4) return 2;
    const int NP = head[0], NPAIR = head[1], n = head[3];
    std::vector<int32_t> pdir(NP), pf(NPAIR), pr(NPAIR);
    std::vector<smx_hit> hits((size_t)n * 2 * NP);
    std::vector<smx_op> ops(n);
    if (fread(pdir.data(), 4, NP, fh) != (size_t)NP || fread(pf.data(), 4, NPAIR, fh) != (size_t)NPAIR ||
        fread(pr.data(), 4, NPAIR, fh) != (size_t)NPAIR || fread(hits.data(), sizeof(smx_hit), hits.size(), fh) != hits.size() ||
        fread(ops.data(), sizeof(smx_op), ops.size(), fh) != ops.size()) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    fclose(fh);
    StatsPanel P = {NP, NPAIR, head[2], pdir.data(), pf.data(), pr.data()};
    uint32_t cap = 8;
    while (cap < (uint32_t)atoi(argv[2])) cap <<= 1;
    const int grid = argc > 3 ? atoi(argv[3]) : 3;
    std::vector<uint64_t> gkeys(cap, SMX_STATS_EMPTY), gcounts(cap, 0);
    uint64_t dropped = 0, spilled = 0;
    auto global_add = [&](uint64_t key, uint64_t add) {
        const int s = stats_find_slot(gkeys.data(), cap, key, cap < STATS_GPROBE_MAX ? cap : STATS_GPROBE_MAX);
        if (s >= 0) gcounts[s] += add; else dropped += add;
    };
    long cands = 0, discarded = 0, filtered = 0, multi = 0;
    std::vector<int> fallback;
    for (int b = 0; b < grid; b++) {   // one "workgroup": its grid-stride share of the reads, then the flush
        std::vector<uint64_t> lkeys(STATS_LCAP, SMX_STATS_EMPTY);
        std::vector<unsigned> lcnt(STATS_LCAP, 0);
        for (long base = (long)b * STATS_THREADS; base < n; base += (long)grid * STATS_THREADS)
            for (long i = base; i < base + STATS_THREADS && i < n; i++) {
                const StatsReadInfo info = stats_read(P, &hits[(size_t)i * 2 * NP], ops[i], [&](uint64_t key) {
                    const int s = stats_find_slot(lkeys.data(), STATS_LCAP, key, STATS_LPROBE);
                    if (s >= 0) lcnt[s]++; else { spilled++; global_add(key, 1); }
                });
                cands += info.n_cand;
                discarded += info.n_discarded;
                filtered += ops[i].rtype == SMX_R_FILTERED;
                multi += ops[i].rtype != SMX_R_FILTERED && ops[i].n_ops > 1;
                if (info.fallback) fallback.push_back((int)i);
            }
        for (int s = 0; s < STATS_LCAP; s++)
            if (lkeys[s] != SMX_STATS_EMPTY && lcnt[s]) global_add(lkeys[s], lcnt[s]);
    }
    if (dropped) {
        printf("SMX_ERR_OVERFLOW the statistics table (%u slots) is full: %llu increments found no slot\n", cap,
               (unsigned long long)dropped);
        return 4;
    }
    long keys = 0;
    for (uint32_t s = 0; s < cap; s++) keys += gkeys[s] != SMX_STATS_EMPTY;
    printf("counters reads=%d candidates=%ld keys=%ld discarded=%ld multi_record=%ld trim_empty=%zu filtered=%ld local_spill=%llu\n",
           n, cands, keys, discarded, multi, fallback.size(), filtered, (unsigned long long)spilled);
    for (int i : fallback) printf("fallback %d\n", i);
    for (uint32_t s = 0; s < cap; s++)
        if (gkeys[s] != SMX_STATS_EMPTY) printf("key %llx %llu\n", (unsigned long long)gkeys[s], (unsigned long long)gcounts[s]);
    return 0;
}
