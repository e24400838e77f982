#!/usr/bin/env python3
"""specimine throughput on a synthetic tree (specimux_amd.synth.write_mine_tree): S specimens x F full x P partial
reads (P per barcode type, both types mined) of ~L nt, all specimens in one mine_specimens() call.  Prints one JSON
line: pairs/s and cell updates/s (sum of len(full) * len(partial) over kernel time, HIP events), end-to-end seconds
(file reading, device work, writing), and a CPU comparator -- a sampled subset through the O(m*n) oracle DP,
extrapolated.  The comparator is that DP, not edlib (edlib is not installed), so no speed-up over edlib is measured.

    python tools/specimine_bench.py [--specimens 96 --full 300 --partial 300 --length 650 --min-identity 0.85]

--run: the whole-run mode.  A plate-grid tree (specimens share forward barcodes, --fwd-groups of them) is mined with
`specimine.mine_run` (what `--run-dir` runs); one JSON line: end-to-end seconds of mine_run, the kernel time and
pairs/s of all its device jobs in one call, and the device memory that call takes, measured in a fresh child process
(device free bytes before / after, workspaces are grow-only)."""
import argparse
import json
import os
import random
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from specimux_amd import _lib, specimine, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--specimens", type=int, default=96)
    ap.add_argument("--full", type=int, default=300)
    ap.add_argument("--partial", type=int, default=300, help="partial reads per barcode type (two types)")
    ap.add_argument("--length", type=int, default=650)
    ap.add_argument("--min-identity", type=float, default=0.85)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-sample", type=int, default=300)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--run", action="store_true", help="whole-run mode (see the module doc)")
    ap.add_argument("--fwd-groups", type=int, default=8, help="--run: forward barcodes shared by the specimens")
    ap.add_argument("--peak", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.peak:
        return peak_child(a)
    if a.run:
        return run_mode(a)
    import ctypes as C
    lib = _lib.load()
    _lib.check(lib.smx_device_init(0, C.byref(C.c_int(0))))
    root = a.workdir or tempfile.mkdtemp(prefix="specimine_bench_")
    t0 = time.perf_counter()
    ids = synth.write_mine_tree(root, a.specimens, a.full, a.partial, a.length, seed=1)
    gen_s = time.perf_counter() - t0
    index = os.path.join(root, "specimens.txt")
    jobs = [specimine.plan_job(index, os.path.join(root, "full", "POOL", f"{s}.fastq"), True, False, a.min_identity)
            for s in ids]
    # pair and cell counts from the inputs
    pairs = cells = 0
    sample_pool = []
    for job in jobs:
        fulls = [r.seq for r in specimine.read_fastq(job.fastq)]
        parts = [r.seq for files in job.partial_files.values() for f in files for r in specimine.read_fastq(f)]
        pairs += len(fulls) * len(parts)
        cells += sum(map(len, fulls)) * sum(map(len, parts))
        sample_pool.append((fulls, parts))
    specimine.mine_specimens(jobs[:1])                       # warm-up: code objects, workspace
    e2e, kms = [], []
    for _ in range(a.repeats):
        ms = []
        t0 = time.perf_counter()
        specimine.mine_specimens(jobs, kernel_ms=ms)
        e2e.append(time.perf_counter() - t0)
        kms.append(sum(ms))
    mined = sum(open(j.output).read().count("\n+\n") for j in jobs)
    # CPU comparator: the oracle's O(m*n) DP on a random sample of the same pairs (k as the tool sets it)
    from oracle.edlib_semantics import HW, align_c
    rng = random.Random(0)
    sample = []
    for _ in range(a.cpu_sample):
        fulls, parts = rng.choice(sample_pool)
        sample.append((rng.choice(fulls), rng.choice(parts)))
    t0 = time.perf_counter()
    for q, t in sample:
        align_c(q, t, HW, specimine.max_distance(len(q), a.min_identity), iupac=False)
    cpu_s = time.perf_counter() - t0
    cpu_rate = len(sample) / cpu_s
    k_ms = min(kms)
    print(json.dumps({
        "bench": "specimine", "specimens": a.specimens, "full_per_specimen": a.full,
        "partial_per_specimen": 2 * a.partial, "read_length": a.length, "min_identity": a.min_identity,
        "pairs": pairs, "cells": cells, "mined_records": mined,
        "kernel_ms": round(k_ms, 3), "pairs_per_s": round(pairs / (k_ms / 1e3), 1),
        "cell_updates_per_s": round(cells / (k_ms / 1e3), 1),
        "e2e_s": round(min(e2e), 3), "e2e_pairs_per_s": round(pairs / min(e2e), 1), "tree_generation_s": round(gen_s, 1),
        "cpu_comparator": "O(mn) DP, not edlib (oracle/align_oracle.c, one core, sampled)",
        "cpu_sample_pairs": len(sample), "cpu_pairs_per_s": round(cpu_rate, 1),
        "cpu_extrapolated_s": round(pairs / cpu_rate, 1),
    }))


def run_jobs(root, min_identity):
    index = os.path.join(root, "specimens.txt")
    return [specimine.plan_job(index, f, True, False, min_identity) for f in specimine.discover_specimens(root, "pool")]


def peak_child(a):
    """Every job of the tree in one call, in a fresh process: device bytes it took."""
    import ctypes as C
    import torch
    lib = _lib.load()
    _lib.check(lib.smx_device_init(0, C.byref(C.c_int(0))))
    jobs = run_jobs(a.workdir, a.min_identity)
    free0, _ = torch.cuda.mem_get_info(0)
    specimine._mine_call(jobs)
    free1, _ = torch.cuda.mem_get_info(0)
    print(json.dumps({"peak_device_bytes": free0 - free1}))


def run_mode(a):
    import ctypes as C
    import subprocess
    lib = _lib.load()
    _lib.check(lib.smx_device_init(0, C.byref(C.c_int(0))))
    root = a.workdir or tempfile.mkdtemp(prefix="specimine_run_bench_")
    ids = synth.write_mine_tree(root, a.specimens, a.full, a.partial, a.length, seed=1, fwd_groups=a.fwd_groups)
    index = os.path.join(root, "specimens.txt")
    jobs = run_jobs(root, a.min_identity)
    pairs = 0
    for job in jobs:
        nf = len(specimine.read_fastq(job.fastq))
        pairs += nf * sum(len(specimine.read_fastq(f)) for f in specimine.job_partials(job))
    specimine._mine_call(jobs[:1])                             # warm-up: code objects, workspace
    e2e, kms = [], []
    for _ in range(a.repeats):
        ms = []
        t0 = time.perf_counter()
        res = specimine.mine_run(root, index, "pool", True, False, a.min_identity)
        e2e.append(time.perf_counter() - t0)
        specimine._mine_call(jobs, kernel_ms=ms)
        kms.append(sum(ms))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--peak", "--workdir", root,
                        "--min-identity", repr(a.min_identity)], capture_output=True, text=True, timeout=900)
    peak = json.loads(r.stdout.strip().splitlines()[-1])["peak_device_bytes"] if r.returncode == 0 else None
    k_ms = min(kms)
    print(json.dumps({
        "bench": "specimine_run", "specimens": len(ids), "fwd_groups": a.fwd_groups, "full_per_specimen": a.full,
        "partial_per_file": a.partial, "read_length": a.length, "min_identity": a.min_identity,
        "pairs": pairs, "mined_specimens": res["mined"], "mined_records": res["reads"],
        "run_dir_e2e_s": round(min(e2e), 3),
        "kernel_ms": round(k_ms, 3), "pairs_per_s": round(pairs / (k_ms / 1e3), 1), "peak_device_bytes": peak,
    }))


if __name__ == "__main__":
    main()
