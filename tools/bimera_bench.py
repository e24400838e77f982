#!/usr/bin/env python3
"""smx_prefix_reach (specimux-bimera's kernel) on a synthetic plate and on the plate against a pool of extra parents.
Sequences of ~L nt: T templates, every called sequence a copy of one at 1 % error (so every sequence has a few close
relatives on the plate, and the rest are strangers); sizes 3..400 reads, need = 2 x size; E = max_edits + min_gain = 5.

    plate   the N sequences against themselves, one job: `--scope plate`
    pool    the N sequences against P extra parents of 600-700 nt (1 % hold a called sequence at up to 3 % error, the
            rest are unrelated), eligible for every query: one call over the whole pool

Per shape one JSON line: kernel ms (HIP events; min / median / max over the repeats after one warm-up call), the
eligible (pair, side) items the call ran, ns per item, and how many (query, side, e) slot pairs came back with two keys.
Between calls the pool is rotated by a seventh of its records.  `--tool` adds the end-to-end time of
`python -m specimux_amd.bimera --scope plate` on the plate's FASTA.  `--out` also writes the lines to a file.

    python tools/bimera_bench.py [--sequences 2000 --parents 100000 --length 650 --repeats 5 --tool --out profiles/bimera.txt]"""
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
sys.path.insert(0, os.path.join(REPO, "tools"))

from specimux_amd import _lib, bimera, calls  # noqa: E402
from cluster_bench import BASES, device_ms, mutate, spread  # noqa: E402


def rand(rng, n):
    return BASES[rng.integers(0, 4, int(n))]


def make_plate(rng, n, length, templates):
    t = [rand(rng, length * rng.uniform(0.97, 1.03)) for _ in range(templates)]
    seqs = [mutate(rng, t[i % templates], 0.01).tobytes() for i in range(n)]
    sizes = [int(x) for x in rng.integers(3, 401, n)]
    return seqs, sizes


def make_pool(rng, seqs, n, lo=600, hi=700, related_share=0.01):
    out = []
    for _ in range(n):
        if rng.random() >= related_share:
            out.append(rand(rng, rng.integers(lo, hi + 1)).tobytes())
        else:
            q = np.frombuffer(seqs[int(rng.integers(0, len(seqs)))], dtype=np.uint8)
            out.append(mutate(rng, q, rng.uniform(0.0, 0.03)).tobytes())
    return out


def reach_call(seqs, sizes, pool, E):
    """-> call(r) -> kernel ms with the pool rotated r times; stats() of the last output"""
    N, P = len(seqs), len(pool)
    job = (0, N, N, P) if P else (0, N, 0, N)
    jarr = calls.job_array([job], _lib.REACH_JOB_DTYPE)
    keys = np.zeros(N * 2 * (E + 1) * bimera.SLOTS, dtype=np.uint64)
    weight = np.array(list(sizes) + [bimera.ALWAYS] * P, dtype=np.uint32)
    need = np.array([bimera.need_of(s, 2000) for s in sizes] + [0] * P, dtype=np.uint32)
    w, nd = weight[:N].astype(np.int64), need[:N].astype(np.int64)
    items = 2 * (N * P if P else int((w[None, :] >= nd[:, None]).sum() - (w >= nd).sum()))

    def call(r):
        at = (r * (P // 7 + 1)) % max(P, 1)
        all_seqs = list(seqs) + pool[at:] + pool[:at]
        return device_ms("smx_prefix_reach", b"".join(all_seqs), _lib.ptr(calls.offsets(all_seqs)), len(all_seqs), _lib.ptr(weight),
                         _lib.ptr(need), _lib.ptr(jarr), 1, E, _lib.ptr(keys))

    def stats():
        pairs = keys.reshape(-1, bimera.SLOTS) != np.uint64(bimera.NONE)
        full = keys.reshape(N, 2, E + 1, bimera.SLOTS)[:, 0, E, 0]
        lens = np.array([len(s) for s in seqs], dtype=np.uint64)
        return {"slot_pairs": int(pairs.shape[0]), "slot_pairs_with_two_keys": int(pairs.all(axis=1).sum()),
                "queries_without_parents": int((~pairs[:, 0].reshape(N, -1)[:, 0]).sum()),
                "queries_explained_by_one_parent": int(((np.uint64(0xFFFFFFFF) - (full >> np.uint64(32))) == lens).sum())}
    return call, stats, items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=2000)
    ap.add_argument("--parents", type=int, default=100000)
    ap.add_argument("--length", type=int, default=650)
    ap.add_argument("--templates", type=int, default=250)
    ap.add_argument("--max-edits", type=int, default=2)
    ap.add_argument("--min-gain", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="plate,pool")
    ap.add_argument("--tool", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import ctypes as C
    lib = _lib.load()
    _lib.check(lib.smx_device_init(0, C.byref(C.c_int(0))))
    rng = np.random.default_rng(1)
    E = a.max_edits + a.min_gain
    seqs, sizes = make_plate(rng, a.sequences, a.length, a.templates)
    lines = []

    def emit(line):
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    base = {"bench": "prefix_reach", "sequences": a.sequences, "length": [min(map(len, seqs)), max(map(len, seqs))],
            "templates": a.templates, "E": E, "repeats": a.repeats}
    for shape in a.shapes.split(","):
        pool = make_pool(rng, seqs, a.parents) if shape == "pool" else []
        call, stats, items = reach_call(seqs, sizes, pool, E)
        ms = [call(r) for r in range(a.repeats + 1)][1:]
        emit(dict(base, shape=shape, parents=len(pool), items=items, **spread(ms),
                  ns_per_item=round(statistics.median(ms) * 1e6 / max(items, 1), 4), **stats()))
    if a.tool:
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "plate.fasta")
            with open(src, "w") as fh:
                for i, (s, size) in enumerate(zip(seqs, sizes)):
                    fh.write(f">W{i % 96:02d}_c{i // 96 + 1} size={size}\n{s.decode()}\n")
            args = bimera.build_parser().parse_args(["--fasta", src, "--scope", "plate", "--max-edits", str(a.max_edits),
                                                     "--min-gain", str(a.min_gain), "--report", os.path.join(d, "r.tsv"),
                                                     "--json", os.path.join(d, "r.json"), "--clean", os.path.join(d, "c.fasta")])
            walls, kms = [], []
            for _ in range(3):
                ms, t0 = [], time.perf_counter()
                assert bimera.run(args, kernel_ms=ms) == 0
                walls.append(round(time.perf_counter() - t0, 3))
                kms.append(round(sum(ms), 3))
            with open(os.path.join(d, "r.json")) as fh:
                summary = json.load(fh)["summary"]
        emit({"bench": "bimera_tool", "shape": "plate", "wall_s": walls, "kernel_ms": kms, "summary": summary})
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
