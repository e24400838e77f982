#!/usr/bin/env python3
"""smx_nj (specimux-tree's kernels) on random integer distance matrices of n = 768, 4 096 and 16 384 tips: a plate, a
few plates and a season's plates in one tree.  Entries 1..3000, no structure: every iteration scans the whole live
triangle.

Per n one JSON line: the call's device time (HIP events around all of its 1 + 2 (n - 3) launches; min / median / max over
the repeats after one warm-up call of the same n -- of n = 4 096 for the largest, whose code objects and workspace path
are the same), the launches, the bytes the row-minimum kernel reads in the call -- 8 bytes of the matrix per live pair
and iteration, sum over na = n .. 4 of na (na - 1) / 2; it reads one r[hi] beside each, which the caches serve -- and
those matrix bytes over the call's whole device time, a lower bound of that kernel's own rate.  `--twin` adds, for context
only, the time of the numpy twin (tests/tree_utils.py nj_reference) at n = 768 on this host.  `--out` also writes the
lines to a file.  No time here is a pass mark.

    python tools/tree_bench.py [--sizes 768,4096,16384 --repeats 5,3,1 --twin --out profiles/tree.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from specimux_amd import _lib, calls  # noqa: E402
from cluster_bench import spread  # noqa: E402


def random_triangle(rng, n):
    return rng.integers(1, 3001, size=n * (n - 1) // 2, dtype=np.int32)


def rowmin_matrix_bytes(n):
    """8 bytes per live pair and iteration: the sum over na = n .. 4 of na (na - 1) / 2 doubles."""
    return 8 * sum(na * (na - 1) // 2 for na in range(4, n + 1))


def nj_ms(tri, n):
    ms = []
    merges, last, _ = calls.nj(tri, n, ms)
    assert len(merges) == n - 3 and int(merges[-1]["n_active"]) == 4 and int(last.max()) < 2 * n - 3
    return ms[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="768,4096,16384")
    ap.add_argument("--repeats", default="5,3,1")
    ap.add_argument("--twin", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import ctypes as C
    lib = _lib.load()
    _lib.check(lib.smx_device_init(0, C.byref(C.c_int(0))))
    rng = np.random.default_rng(1)
    sizes = [int(x) for x in a.sizes.split(",")]
    repeats = [int(x) for x in a.repeats.split(",")]
    lines = []

    def emit(line):
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    warmed = 0
    for n, reps in zip(sizes, repeats):
        tri = random_triangle(rng, n)
        if n <= 4096 or not warmed:
            nj_ms(tri, n)
            warmed = n
        ms = [nj_ms(tri, n) for _ in range(reps)]
        b = rowmin_matrix_bytes(n)
        emit(dict({"bench": "nj", "n": n, "repeats": reps, "warm_up_n": warmed, "launches": 1 + 2 * (n - 3),
                   "rowmin_matrix_bytes": b, "rowmin_matrix_GB_per_s_over_call": round(b / (min(ms) * 1e-3) / 1e9, 1),
                   "us_per_iteration": round(min(ms) * 1e3 / (n - 3), 2)}, **spread(ms)))
        del tri
    if a.twin:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import tree_utils
        D = tree_utils.full_of(random_triangle(rng, 768), 768)
        t0 = time.perf_counter()
        tree_utils.nj_reference(D)
        emit({"bench": "nj_numpy_twin_for_context_only", "n": 768, "host_wall_s": round(time.perf_counter() - t0, 3)})
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
