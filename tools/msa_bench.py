#!/usr/bin/env python3
"""smx_msa (specimux-msa's kernels) on synthetic runs of n = 96, 768 and 4 096 sequences of about 650 nt, each 0-15 % away
from one ancestor (substitutions, and an insertion or a deletion per 100 differences or so), on a balanced guide tree
(log2 n levels, n / 2 merges in the widest) and on a ladder (n - 1 levels of one merge: the latency of a single merge).

Per shape one JSON line: the call's device time (HIP events, summed over the call's launches; min / median / max over the
repeats after one warm-up call), the levels, the mean time per merge, the columns of the root and the DP cells of the call
(the sum over the merges of La x Lb, from the returned lengths); then, from smx_msa_debug_times after one more call with
SMX_MSA_PHASE_TIMING set: the device time of every level (all of them for a balanced tree; first, last, min, median and
max for a ladder), of the tips and the rows launch, and the share of the merge kernel's three phases -- forward, walk back,
build -- in the time its workgroups were resident (thread 0's wall-clock reads at the phase barriers, summed over the
merges).  `--host` compiles tests/cpu/msa_sim.cpp and times the host loops of tests/cpu/msa_host.h on the smallest shape;
`--twin` adds the numpy twin (tests/msa_utils.py msa_reference) there.  Both are for scale only.  `--out` also writes the
lines to a file.  No time here is a pass mark.

    python tools/msa_bench.py [--sizes 96,768,4096 --repeats 5,3,1 --host --twin --out profiles/msa.txt]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from specimux_amd import _lib, calls  # noqa: E402
from cluster_bench import spread  # noqa: E402
import msa_utils  # noqa: E402


def synthetic_run(rng, n, length=650, most=0.15):
    ancestor = rng.integers(0, 4, size=length)
    out = []
    for _ in range(n):
        s = ancestor.copy()
        hit = rng.random(length) < rng.random() * most
        s[hit] = (s[hit] + rng.integers(1, 4, size=int(hit.sum()))) % 4
        for _ in range(int(hit.sum()) // 100 + int(rng.integers(0, 2))):
            at = int(rng.integers(1, len(s) - 1))
            s = np.delete(s, at) if rng.random() < 0.5 else np.insert(s, at, rng.integers(0, 4))
        out.append(bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[s].tolist()))
    return out


def cells_of(seqs, merges, lens):
    length = [len(s) for s in seqs] + [int(x) for x in lens]
    return sum(length[a] * length[b] for a, b in merges)


def debug_times(levels):
    """smx_msa_debug_times of the last call: (level_ms, tips_ms, rows_ms, phase_us)."""
    level_ms = np.zeros(max(levels, 1), dtype=np.float32)
    n_levels, tips_rows, phase_us = np.zeros(1, dtype=np.uint32), np.zeros(2, dtype=np.float32), np.zeros(3, dtype=np.float64)
    _lib.check(_lib.load().smx_msa_debug_times(_lib.ptr(level_ms), levels, _lib.ptr(n_levels), _lib.ptr(tips_rows), _lib.ptr(phase_us)))
    assert int(n_levels[0]) == levels
    return level_ms[:levels].tolist(), float(tips_rows[0]), float(tips_rows[1]), phase_us.tolist()


def host_loops(n):
    """The wall time of tests/cpu/msa_host.h's loops (msa_sim time n), compiled here with g++ -O2."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "msa_sim")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "specimux_amd", "csrc"), "-I",
                               os.path.join(REPO, "include"), "-I", os.path.join(REPO, "tests", "cpu"), "-o", exe,
                               os.path.join(REPO, "tests", "cpu", "msa_sim.cpp")])
        words = subprocess.run([exe, "time", str(n)], capture_output=True, text=True, check=True).stdout.split()
    return dict(zip(words[1::2], words[2::2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="96,768,4096")
    ap.add_argument("--repeats", default="5,3,1")
    ap.add_argument("--twin", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    lib = _lib.load()
    _lib.check(lib.smx_device_init(0, C.byref(C.c_int(0))))
    rng = np.random.default_rng(1)
    sizes = [int(x) for x in a.sizes.split(",")]
    repeats = [int(x) for x in a.repeats.split(",")]
    lines = []

    def emit(line):
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    smallest = None
    for n, reps in zip(sizes, repeats):
        seqs = synthetic_run(rng, n)
        smallest = smallest or seqs
        for shape, merges, levels in (("balanced", msa_utils.balanced_tree(n), int(np.ceil(np.log2(n)))),
                                      ("ladder", msa_utils.ladder_tree(n), n - 1)):
            ms, wall = [], []
            for rep in range(reps + 1):               # the first is the warm-up
                one = []
                t0 = time.perf_counter()
                rows, lens, costs = calls.msa(seqs, merges, kernel_ms=one)
                wall.append(time.perf_counter() - t0)
                if rep:
                    ms.append(sum(one))
            assert rows.shape[0] == n and all(bytes(r[r != 45].tolist()) == s for r, s in list(zip(rows, seqs))[:8])
            cells = cells_of(seqs, merges, lens)
            os.environ["SMX_MSA_PHASE_TIMING"] = "1"       # one more call, with the phase clocks: not among the timed ones
            try:
                timed_ms = []
                calls.msa(seqs, merges, kernel_ms=timed_ms)
            finally:
                del os.environ["SMX_MSA_PHASE_TIMING"]
            level_ms, tips_ms, rows_ms, phase_us = debug_times(levels)
            resident = sum(phase_us) or 1.0
            per_level = ({"level_ms": [round(x, 3) for x in level_ms]} if shape == "balanced" else
                         {"level_ms_first": round(level_ms[0], 3), "level_ms_last": round(level_ms[-1], 3),
                          "level_ms_min": round(min(level_ms), 3), "level_ms_median": round(statistics.median(level_ms), 3),
                          "level_ms_max": round(max(level_ms), 3)})
            emit(dict({"bench": "msa", "n": n, "tree": shape, "repeats": reps, "levels": levels, "merges": n - 1,
                       "root_columns": int(rows.shape[1]), "dp_cells": cells, "sum_of_pairs": int(costs.sum(dtype=np.uint64)),
                       "us_per_merge": round(min(ms) * 1e3 / (n - 1), 2),
                       "Gcells_per_s": round(cells / (min(ms) * 1e-3) / 1e9, 3), "call_wall_s_min": round(min(wall[1:]), 4)},
                      **spread(ms), **per_level, tips_ms=round(tips_ms, 3), rows_ms=round(rows_ms, 3),
                      phase_timed_call_ms=round(sum(timed_ms), 3),
                      phase_share={k: round(v / resident, 3) for k, v in zip(("forward", "walk", "build"), phase_us)},
                      phase_us_per_merge={k: round(v / (n - 1), 1) for k, v in zip(("forward", "walk", "build"), phase_us)}))
    if a.host:
        emit(dict({"bench": "msa_host_loops_for_scale_only", "tree": "balanced"}, **host_loops(len(smallest))))
    if a.twin:
        merges = msa_utils.balanced_tree(len(smallest))
        t0 = time.perf_counter()
        msa_utils.msa_reference(smallest, merges)
        emit({"bench": "msa_numpy_twin_for_context_only", "n": len(smallest), "tree": "balanced",
              "host_wall_s": round(time.perf_counter() - t0, 3)})
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
