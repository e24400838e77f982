#!/usr/bin/env python3
"""smx_cons_resample against smx_cons_votes on a synthetic plate: C clusters x R reads of ~L nt with per-read error E,
every cluster's reads aligned to its template in one call, and the vote taken again over 64 subsets at each of 8 levels
(the half sample and the tool's default depths, subsets as the tool draws them).  The two calls alternate, five each
after a warm-up, timed with HIP events.  Then the tool itself, from a run directory to its four files.  Prints JSON lines:

  cons_votes      kernel ms of smx_cons_votes (min / median / max over the repeats)
  cons_resample   kernel ms of smx_cons_resample over the same jobs: the same alignment and vote, then
                  cons_resample_kernel over the rows; the replicates that reproduce the template per level
  difference      the medians' difference and ratio: what 8 x 64 = 512 resampled votes per cluster cost over one
                  alignment pass, and the rate in (member, column, replicate) counts per second
  tool            wall seconds of specimux-support over a tree of the same shape (clusters, consensus and the resampling)

    python tools/support_bench.py [--clusters 96 --reads 500 --length 650 --error 0.05 --min-identity 0.85 --repeats 5]
        [--no-tool]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cluster_bench import BASES, device_ms, mutate, spread, timed, write_tree  # noqa: E402
from specimux_amd import _lib, calls, specimine, support  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=96)
    ap.add_argument("--reads", type=int, default=500)
    ap.add_argument("--length", type=int, default=650)
    ap.add_argument("--error", type=float, default=0.05)
    ap.add_argument("--min-identity", type=float, default=0.85)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--depths", default=support.DEFAULT_DEPTHS)
    ap.add_argument("--no-tool", action="store_true")
    a = ap.parse_args()
    import ctypes as C
    lib = _lib.load()
    _lib.check(lib.smx_device_init(0, C.byref(C.c_int(0))))
    rng = np.random.default_rng(1)
    depths = support.parse_depths(a.depths)
    n_levels = 1 + len(depths)
    reads, jobs = [], []
    for c in range(a.clusters):
        template = BASES[rng.integers(0, 4, int(a.length * rng.uniform(0.95, 1.05)))]
        first = len(reads)
        for _ in range(a.reads):
            reads.append(mutate(rng, template, a.error).tobytes())
        reads.append(template.tobytes())                       # the draft: not a member
        jobs.append((first + a.reads, first, a.reads))
    ks = [specimine.max_distance(len(r), a.min_identity) for r in reads]
    masks = np.empty((n_levels, a.clusters * a.reads), dtype=np.uint64)
    for c in range(a.clusters):
        for l, (tag, d, _) in enumerate(support.level_depths(a.reads, depths)):
            masks[l, c * a.reads:(c + 1) * a.reads] = support.subset_masks(1, f"S{c:03d}_c1", tag, a.reads, d)
    roff, karr, jarr = calls.offsets(reads), calls.limits(ks), calls.job_array(jobs, _lib.CONS_JOB_DTYPE)
    votes = np.zeros(sum((len(reads[d]) + 1) * _lib.CONS_VOTE_WORDS for d, _, _ in jobs), dtype=np.uint32)
    aligned = np.zeros(a.clusters, dtype=np.uint32)
    blob = b"".join(reads)

    def votes_call():
        return device_ms("smx_cons_votes", blob, _lib.ptr(roff), len(reads), _lib.ptr(karr), _lib.ptr(jarr), a.clusters,
                         _lib.ptr(votes), _lib.ptr(aligned))

    last = []

    def resample_call():
        ms = []
        last[:] = support.resample(reads, ks, jobs, masks, ms)
        return ms[0]

    v_ms, r_ms = timed([votes_call, resample_call], a.repeats)
    shape = {"clusters": a.clusters, "reads_per_cluster": a.reads, "read_length": a.length, "error": a.error,
             "min_identity": a.min_identity, "repeats": a.repeats, "levels": n_levels, "depths": depths}
    n_align = a.clusters * a.reads
    print(json.dumps(dict({"bench": "cons_votes"}, **shape, alignments=n_align, aligned=int(aligned.sum()), **spread(v_ms))), flush=True)
    whole = [[support.level_numbers(js.agree[l], js.sub_aligned[l])[1] for js in last] for l in range(n_levels)]
    columns = sum(js.agree.shape[1] for js in last)
    print(json.dumps(dict({"bench": "cons_resample"}, alignments=n_align, aligned=sum(js.aligned for js in last),
                          agree_words=columns * n_levels,
                          replicates_reproducing_per_level=[round(statistics.mean(w), 1) for w in whole],
                          **spread(r_ms))), flush=True)
    vm, rm = statistics.median(v_ms), statistics.median(r_ms)
    counts = sum(js.agree.shape[1] * n for js, (_, _, n) in zip(last, jobs)) * n_levels * support.REPLICATES
    print(json.dumps({"bench": "difference", "resample_minus_votes_ms": round(rm - vm, 3), "resample_over_votes": round(rm / vm, 3),
                      "member_column_replicate_counts": counts,
                      "counts_per_second": round(counts / max(rm - vm, 1e-6) * 1e3)}), flush=True)
    if a.no_tool:
        return
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, a.clusters, a.reads, a.length, a.error)
        out = os.path.join(root, "support")
        argv = ["--run-dir", root, "--min-identity", str(a.min_identity), "--depths", a.depths, "--report", out + ".tsv",
                "--json", out + ".json", "--columns", out + ".columns.tsv", "--masked", out + ".fasta"]
        kernel_ms = []
        t0 = time.perf_counter()
        status = support.run(support.build_parser().parse_args(argv), kernel_ms=kernel_ms)
        wall = time.perf_counter() - t0
        with open(out + ".json") as fh:
            summary = json.load(fh)["summary"]
    print(json.dumps({"bench": "tool", "status": status, "wall_s": round(wall, 2), "kernel_ms_total": round(sum(kernel_ms), 1),
                      "sequences": summary["sequences"], "solid": summary["solid"], "weak": summary["weak"],
                      "unconverged": summary["unconverged"], "resample_calls": summary["resample_calls"]}), flush=True)


if __name__ == "__main__":
    main()
