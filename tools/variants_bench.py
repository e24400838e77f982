#!/usr/bin/env python3
"""smx_cons_phase against smx_cons_votes on a synthetic plate: C clusters x R reads of ~L nt with per-read error E, a
second allele planted at three sites in a third of each cluster's reads, every cluster's reads aligned to its template
in one call.  The two calls alternate, five each after a warm-up, timed with HIP events.  Prints JSON lines:

  cons_votes   kernel ms of smx_cons_votes (min / median / max over the repeats)
  cons_phase   kernel ms of smx_cons_phase over the same arguments: the same alignment and vote, then the site, plane and
               link kernels; the sites kept, how many of the planted sites were found and linked
  difference   the medians' difference and ratio: what the second pass over the rows costs.  The forward pass writes
               about 31 KB of history per alignment and a row is 2.6 KB, so a ratio above 2 is a defect, not a figure

    python tools/variants_bench.py [--clusters 96 --reads 500 --length 650 --error 0.05 --min-identity 0.85 --repeats 5]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cluster_bench import BASES, device_ms, mutate, spread, timed  # noqa: E402
from specimux_amd import _lib, calls, specimine, variants  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=96)
    ap.add_argument("--reads", type=int, default=500)
    ap.add_argument("--length", type=int, default=650)
    ap.add_argument("--error", type=float, default=0.05)
    ap.add_argument("--min-identity", type=float, default=0.85)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-sites", type=int, default=32)
    a = ap.parse_args()
    import ctypes as C
    lib = _lib.load()
    _lib.check(lib.smx_device_init(0, C.byref(C.c_int(0))))
    rng = np.random.default_rng(1)
    reads, ks, jobs, planted = [], [], [], []
    for c in range(a.clusters):
        template = BASES[rng.integers(0, 4, int(a.length * rng.uniform(0.95, 1.05)))]
        sites = sorted(int(p) for p in rng.choice(template.size, 3, replace=False))
        other = template.copy()
        for p in sites:
            other[p] = BASES[(int(np.nonzero(BASES == template[p])[0][0]) + 1) % 4]
        first = len(reads)
        for i in range(a.reads):
            reads.append(mutate(rng, other if i % 3 == 0 else template, a.error).tobytes())
        reads.append(template.tobytes())                       # the draft: not a member
        jobs.append((first + a.reads, first, a.reads))
        planted.append(sites)
    ks = [specimine.max_distance(len(r), a.min_identity) for r in reads]
    roff, karr, jarr = calls.offsets(reads), calls.limits(ks), calls.job_array(jobs, _lib.CONS_JOB_DTYPE)
    votes = np.zeros(sum((len(reads[d]) + 1) * _lib.CONS_VOTE_WORDS for d, _, _ in jobs), dtype=np.uint32)
    aligned = np.zeros(a.clusters, dtype=np.uint32)
    blob = b"".join(reads)

    def votes_call():
        return device_ms("smx_cons_votes", blob, _lib.ptr(roff), len(reads), _lib.ptr(karr), _lib.ptr(jarr), a.clusters,
                         _lib.ptr(votes), _lib.ptr(aligned))

    last = []

    def phase_call():
        ms = []
        last[:] = variants.phase(reads, ks, jobs, 150, 5, a.max_sites, ms)
        return ms[0]

    v_ms, p_ms = timed([votes_call, phase_call], a.repeats)
    found = linked = 0
    for jp, sites in zip(last, planted):
        at = {s.pos: i for i, s in enumerate(jp.sites) if s.kind == 0}
        found += sum(p in at for p in sites)
        partners, _ = variants.accept_sites(jp.sites, jp.link, jp.aligned, 5, 500, 300)
        linked += sum(p in at and bool(partners[at[p]]) for p in sites)
    shape = {"clusters": a.clusters, "reads_per_cluster": a.reads, "read_length": a.length, "error": a.error,
             "min_identity": a.min_identity, "repeats": a.repeats, "max_sites": a.max_sites}
    n_align = a.clusters * a.reads
    print(json.dumps(dict({"bench": "cons_votes"}, **shape, alignments=n_align, aligned=int(aligned.sum()), **spread(v_ms))), flush=True)
    print(json.dumps(dict({"bench": "cons_phase"}, alignments=n_align, aligned=sum(jp.aligned for jp in last),
                          sites_kept=sum(len(jp.sites) for jp in last), sites_qualified=sum(jp.n_qualified for jp in last),
                          planted=3 * a.clusters, planted_found=found, planted_linked=linked, **spread(p_ms))), flush=True)
    vm, pm = statistics.median(v_ms), statistics.median(p_ms)
    print(json.dumps({"bench": "difference", "phase_minus_votes_ms": round(pm - vm, 3), "phase_over_votes": round(pm / vm, 3),
                      "row_bytes_read_again": int(sum(4 * n * len(jp.sites) for jp, (_, _, n) in zip(last, jobs)))}), flush=True)


if __name__ == "__main__":
    main()
