#!/usr/bin/env python3
"""smx_cons_votes on a synthetic plate: C clusters x R reads of ~L nt with per-read error E, every cluster's reads
aligned to its first read in one call (one polishing round).  Prints JSON lines:

  cons_votes        kernel ms of smx_cons_votes (HIP events; min / median / max over the repeats after one warm-up call),
                    alignments per second, the share of the members that aligned within their limit, and the history
                    bytes the forward pass writes per alignment (computed from the band: 20 bytes per block and column)
  pairs_neighbours  smx_pairs_neighbours over the same reads (all pairs within each cluster), alternating with the
                    call above, as context: kernel ms and pairs per second

    python tools/consensus_bench.py [--clusters 96 --reads 500 --length 650 --error 0.05 --min-identity 0.85 --repeats 5]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cluster_bench import BASES, device_ms, mutate, pairs_call, spread, timed  # noqa: E402
from specimux_amd import _lib, calls, specimine  # noqa: E402


def history_bytes(m, n, k):
    """Bytes one alignment that runs to its last column leaves in the history: per column the blocks F..L of
    smx_cons_core.h's band, 16 bytes of (Pv, Mv) and 4 of bottom score each."""
    if k < 0 or k > max(m, n):
        k = max(m, n)
    g = m - n
    if abs(g) > k or not m or not n:
        return 0
    e = (k - abs(g)) >> 1
    dlo, dhi = min(g, 0) - e, max(g, 0) + e
    j = np.arange(n)
    first = np.maximum(j + dlo, 0) >> 6
    last = np.minimum((m + 63) // 64 - 1, (j + dhi) >> 6)
    return int((last - first + 1).sum()) * 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=96)
    ap.add_argument("--reads", type=int, default=500)
    ap.add_argument("--length", type=int, default=650)
    ap.add_argument("--error", type=float, default=0.05)
    ap.add_argument("--min-identity", type=float, default=0.85)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import ctypes as C
    lib = _lib.load()
    _lib.check(lib.smx_device_init(0, C.byref(C.c_int(0))))
    rng = np.random.default_rng(1)
    specimens = []
    for _ in range(a.clusters):
        template = BASES[rng.integers(0, 4, int(a.length * rng.uniform(0.95, 1.05)))]
        reads = [mutate(rng, template, a.error).tobytes() for _ in range(a.reads)]
        specimens.append((reads, [specimine.max_distance(len(r), a.min_identity) for r in reads]))
    reads = [r for rs, _ in specimens for r in rs]
    roff = calls.offsets(reads)
    karr = calls.limits([k for _, ks in specimens for k in ks])
    jobs = calls.job_array([(c * a.reads, c * a.reads, a.reads) for c in range(a.clusters)], _lib.CONS_JOB_DTYPE)
    votes = np.zeros(sum((len(rs[0]) + 1) * _lib.CONS_VOTE_WORDS for rs, _ in specimens), dtype=np.uint32)
    aligned = np.zeros(a.clusters, dtype=np.uint32)
    blob = b"".join(reads)

    def cons_call():
        return device_ms("smx_cons_votes", blob, _lib.ptr(roff), len(reads), _lib.ptr(karr), _lib.ptr(jobs), a.clusters,
                         _lib.ptr(votes), _lib.ptr(aligned))

    nb_call, nb_count = pairs_call(specimens, True)
    c_ms, n_ms = timed([cons_call, nb_call], a.repeats)
    n_align = a.clusters * a.reads
    hist = [history_bytes(len(rs[0]), len(r), max(ks[0], k)) for rs, ks in specimens for r, k in zip(rs, ks)]
    shape = {"clusters": a.clusters, "reads_per_cluster": a.reads, "read_length": a.length, "error": a.error,
             "min_identity": a.min_identity, "repeats": a.repeats}
    print(json.dumps(dict({"bench": "cons_votes"}, **shape, alignments=n_align, aligned=int(aligned.sum()), **spread(c_ms),
                          alignments_per_s=round(n_align / (statistics.median(c_ms) / 1e3), 1),
                          history_bytes_per_alignment=round(sum(hist) / n_align, 1),
                          history_gb_per_call=round(sum(hist) / 1e9, 3))), flush=True)
    pairs = a.clusters * a.reads * (a.reads - 1) // 2
    print(json.dumps(dict({"bench": "pairs_neighbours"}, pairs=pairs, within_limit=nb_count(), **spread(n_ms),
                          pairs_per_s=round(pairs / (statistics.median(n_ms) / 1e3), 1))), flush=True)


if __name__ == "__main__":
    main()
