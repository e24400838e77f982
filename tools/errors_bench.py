#!/usr/bin/env python3
"""smx_cons_profile against smx_cons_votes on a synthetic plate: C clusters x R reads of ~L nt with per-read error E and
random quality bytes, every cluster's reads aligned to its template in one call, and the rows reduced to the error
profile.  The two calls alternate, five each after a warm-up, timed with HIP events.  Then the tool itself, from a run
directory to its five files.  Prints JSON lines:

  cons_votes      kernel ms of smx_cons_votes (min / median / max over the repeats)
  cons_profile    kernel ms of smx_cons_profile over the same jobs: the same alignment and vote, then cons_profile_kernel
                  over the rows; the measured rates per 1 000 bases, to be held against the planted error
  difference      the medians' difference and ratio: what the profile kernel costs over one alignment pass, and the row
                  words it reads per second
  tool            wall seconds of specimux-errors over a tree of the same shape (clusters, consensus and the profile)

    python tools/errors_bench.py [--clusters 96 --reads 500 --length 650 --error 0.05 --min-identity 0.85 --repeats 5]
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
from specimux_amd import _lib, calls, errors, specimine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=96)
    ap.add_argument("--reads", type=int, default=500)
    ap.add_argument("--length", type=int, default=650)
    ap.add_argument("--error", type=float, default=0.05)
    ap.add_argument("--min-identity", type=float, default=0.85)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-tool", action="store_true")
    a = ap.parse_args()
    import ctypes as C
    lib = _lib.load()
    _lib.check(lib.smx_device_init(0, C.byref(C.c_int(0))))
    rng = np.random.default_rng(1)
    reads, quals, jobs = [], [], []
    for c in range(a.clusters):
        template = BASES[rng.integers(0, 4, int(a.length * rng.uniform(0.95, 1.05)))]
        first = len(reads)
        for _ in range(a.reads):
            reads.append(mutate(rng, template, a.error).tobytes())
        reads.append(template.tobytes())                       # the draft: not a member
        jobs.append((first + a.reads, first, a.reads))
    for r in reads:
        quals.append((33 + rng.integers(10, 41, len(r))).astype(np.uint8).tobytes())
    ks = [specimine.max_distance(len(r), a.min_identity) for r in reads]
    roff, karr, jarr = calls.offsets(reads), calls.limits(ks), calls.job_array(jobs, _lib.CONS_JOB_DTYPE)
    votes = np.zeros(sum((len(reads[d]) + 1) * _lib.CONS_VOTE_WORDS for d, _, _ in jobs), dtype=np.uint32)
    aligned = np.zeros(a.clusters, dtype=np.uint32)
    blob = b"".join(reads)

    def votes_call():
        return device_ms("smx_cons_votes", blob, _lib.ptr(roff), len(reads), _lib.ptr(karr), _lib.ptr(jarr), a.clusters,
                         _lib.ptr(votes), _lib.ptr(aligned))

    last = []

    def profile_call():
        ms = []
        last[:] = errors.profile(reads, quals, ks, jobs, ms)
        return ms[0]

    v_ms, p_ms = timed([votes_call, profile_call], a.repeats)
    shape = {"clusters": a.clusters, "reads_per_cluster": a.reads, "read_length": a.length, "error": a.error,
             "min_identity": a.min_identity, "repeats": a.repeats}
    n_align = a.clusters * a.reads
    print(json.dumps(dict({"bench": "cons_votes"}, **shape, alignments=n_align, aligned=int(aligned.sum()), **spread(v_ms))), flush=True)
    run = errors.Totals("run")
    for jp in last:
        run.add_job(jp)
    row_words = sum((len(reads[d]) + 1) * n for d, _, n in jobs)
    print(json.dumps(dict({"bench": "cons_profile"}, alignments=n_align, aligned=run.aligned, clipped=run.clipped, row_words=row_words,
                          row_bytes=4 * row_words, bases=run.bases, sub_per_kb=errors.fmt_rate(run.words[errors.SUB], run.bases),
                          ins_per_kb=errors.fmt_rate(run.words[errors.INS_BASES], run.bases),
                          del_per_kb=errors.fmt_rate(run.words[errors.DEL], run.bases), **spread(p_ms))), flush=True)
    vm, pm = statistics.median(v_ms), statistics.median(p_ms)
    print(json.dumps({"bench": "difference", "profile_minus_votes_ms": round(pm - vm, 3), "profile_over_votes": round(pm / vm, 3),
                      "row_words_per_second": round(row_words / max(pm - vm, 1e-6) * 1e3),
                      "row_gbytes_per_second": round(4 * row_words / max(pm - vm, 1e-6) / 1e6, 1)}), flush=True)
    if a.no_tool:
        return
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, a.clusters, a.reads, a.length, a.error)
        out = os.path.join(root, "errors")
        argv = ["--run-dir", root, "--report", out + ".tsv", "--json", out + ".json", "--quality", out + ".quality.tsv",
                "--homopolymers", out + ".hp.tsv", "--reads", out + ".reads.tsv"]
        kernel_ms = []
        t0 = time.perf_counter()
        status = errors.run(errors.build_parser().parse_args(argv), kernel_ms=kernel_ms)
        wall = time.perf_counter() - t0
        with open(out + ".json") as fh:
            doc = json.load(fh)
    print(json.dumps({"bench": "tool", "status": status, "wall_s": round(wall, 2), "kernel_ms_total": round(sum(kernel_ms), 1),
                      "sequences": doc["summary"]["sequences"], "profile_calls": doc["summary"]["profile_calls"],
                      "aligned": doc["run"]["aligned"], "not_aligned": doc["run"]["not_aligned"],
                      "sub_per_kb": doc["run"]["sub_per_kb"], "ins_per_kb": doc["run"]["ins_per_kb"], "del_per_kb": doc["run"]["del_per_kb"],
                      "implied_min_identity": doc["implied"]["min_identity"]}), flush=True)


if __name__ == "__main__":
    main()
