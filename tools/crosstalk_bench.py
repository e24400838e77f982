#!/usr/bin/env python3
"""smx_nearest (specimux-crosstalk's kernel) on a synthetic plate, next to smx_pairs_neighbours on the same reads:
S specimens x R reads of ~L nt at 5 % per-read error, each read limited to 10 % of its length, against two ref sets --
the S templates, and those plus 7 S unrelated sequences (768 refs at S = 96, of which 672 are unrelated).  For every ref
set and every G (the chunks the plan keeps a call above, as a multiple of the device's CU count, through
SMX_NEAREST_MIN_CHUNKS) one JSON line: kernel ms of smx_nearest (HIP events; min / median / max over the repeats after
one warm-up call, alternating with smx_pairs_neighbours), ns per pair, the pairs kernel's ns per pair in the same
rounds, and the reads that found an own / another ref.

    python tools/crosstalk_bench.py [--specimens 96 --reads 500 --length 650 --error 0.05 --min-identity 0.90
                                     --repeats 5 --chunks-per-cu 2,8,32]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from specimux_amd import _lib, calls, specimine  # noqa: E402
from cluster_bench import BASES, device_ms, mutate, pairs_call, spread, timed  # noqa: E402


def nearest_call(seqs, ks, groups, jobs):
    """-> (call() -> kernel ms, found() -> reads with an own key, reads with an other key in the last output)"""
    off, karr, jarr = calls.offsets(seqs), calls.limits(ks), calls.job_array(jobs, _lib.NEAREST_JOB_DTYPE)
    garr = np.array(groups, dtype=np.uint32)
    n = sum(j[3] for j in jobs)
    own, other = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    blob = b"".join(seqs)

    def call():
        return device_ms("smx_nearest", blob, _lib.ptr(off), len(seqs), _lib.ptr(karr), _lib.ptr(garr), _lib.ptr(jarr), len(jobs),
                         _lib.ptr(own), _lib.ptr(other))

    none = np.uint64(2**64 - 1)
    return call, lambda: (int((own != none).sum()), int((other != none).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--specimens", type=int, default=96)
    ap.add_argument("--reads", type=int, default=500)
    ap.add_argument("--length", type=int, default=650)
    ap.add_argument("--error", type=float, default=0.05)
    ap.add_argument("--min-identity", type=float, default=0.90)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunks-per-cu", default="2,8,32")
    a = ap.parse_args()
    import ctypes as C
    import torch
    lib = _lib.load()
    _lib.check(lib.smx_device_init(0, C.byref(C.c_int(0))))
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(1)
    templates = [BASES[rng.integers(0, 4, int(a.length * rng.uniform(0.95, 1.05)))] for _ in range(a.specimens)]
    unrelated = [BASES[rng.integers(0, 4, int(a.length * rng.uniform(0.95, 1.05)))] for _ in range(7 * a.specimens)]
    reads = [[mutate(rng, t, a.error).tobytes() for _ in range(a.reads)] for t in templates]
    k_of = lambda s: specimine.max_distance(len(s), a.min_identity)   # noqa: E731
    specimens = [(rs, [k_of(r) for r in rs]) for rs in reads]
    p_call, p_within = pairs_call(specimens, True)
    tri = sum(len(rs) * (len(rs) - 1) // 2 for rs in reads)
    for refs in (templates, templates + unrelated):
        seqs = [t.tobytes() for t in refs]
        groups = list(range(len(refs)))
        jobs = []
        for s, rs in enumerate(reads):
            jobs.append((0, len(refs), len(seqs), len(rs)))
            seqs += rs
            groups += [s] * len(rs)
        ks = [k_of(s) for s in seqs]
        n_call, found = nearest_call(seqs, ks, groups, jobs)
        pairs = len(refs) * sum(len(rs) for rs in reads)
        for per_cu in [int(x) for x in a.chunks_per_cu.split(",")]:
            os.environ["SMX_NEAREST_MIN_CHUNKS"] = str(per_cu * n_cu)
            n_ms, p_ms = timed([n_call, p_call], a.repeats)
            own, other = found()
            print(json.dumps(dict({"bench": "nearest", "specimens": a.specimens, "reads_per_specimen": a.reads,
                                   "read_length": a.length, "error": a.error, "min_identity": a.min_identity, "refs": len(refs),
                                   "unrelated_refs": len(refs) - a.specimens, "cus": n_cu, "chunks_per_cu": per_cu,
                                   "pairs": pairs}, **spread(n_ms), ns_per_pair=round(statistics.median(n_ms) * 1e6 / pairs, 3),
                                  reads_with_own=own, reads_with_other=other,
                                  pairs_neighbours=dict(spread(p_ms), pairs=tri, within_limit=p_within(),
                                                        ns_per_pair=round(statistics.median(p_ms) * 1e6 / tri, 3)))), flush=True)


if __name__ == "__main__":
    main()
