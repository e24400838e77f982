#!/usr/bin/env python3
"""smx_best_hits (specimux-identify's kernel) on synthetic reference databases, next to smx_mine_best_identity where the
two can run the identical pair set.  Queries of ~L nt from T templates at 2 % error; limits int(len * (1 - min_identity)).

    A   refs of 700-800 nt, every one longer than every query (side Q carries everything): 1 % hold a query at up to 8 %
        error between flanks, the rest are unrelated.  smx_mine_best_identity runs the same pairs with the same
        mine_pair and limits: the yardstick, taken alternately
    B   the same with refs of 450-550 nt, every one shorter than every query (side T carries everything); the related
        1 % are pieces of a query
    C   the queries against themselves: a plate's consensus file against itself, every query with hits

Per shape one JSON line: kernel ms (HIP events; min / median / max over the repeats after one warm-up call), pairs per
second, the queries with a hit and the filled slots.  Between calls the database is rotated by a seventh of its records,
so that no call finds the previous call's bytes at the same addresses.  `--tool` adds the end-to-end time of
`python -m specimux_amd.identify` on shape A: FASTA parse, device calls, reports.

    python tools/identify_bench.py [--queries 768 --refs 100000 --length 650 --top 5 --min-coverage 0.5 --repeats 5 --tool]"""
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

from specimux_amd import _lib, calls, identify, specimine  # noqa: E402
from cluster_bench import BASES, device_ms, mutate, spread  # noqa: E402


def rand(rng, n):
    return BASES[rng.integers(0, 4, int(n))]


def make_queries(rng, n, length, templates):
    t = [rand(rng, length * rng.uniform(0.97, 1.03)) for _ in range(templates)]
    return [mutate(rng, t[i % templates], 0.02).tobytes() for i in range(n)]


def make_refs(rng, queries, n, lo, hi, related_share=0.01):
    """n refs of lo..hi nt.  Longer than the queries: a related ref holds a query at up to 8 % error between flanks.
    Shorter: it is a piece of one."""
    out = []
    for i in range(n):
        m = int(rng.integers(lo, hi + 1))
        if rng.random() >= related_share:
            out.append(rand(rng, m).tobytes())
            continue
        q = mutate(rng, np.frombuffer(queries[int(rng.integers(0, len(queries)))], dtype=np.uint8), rng.uniform(0.0, 0.08))
        if m > q.size:
            left = int(rng.integers(0, m - q.size + 1))
            out.append(np.concatenate([rand(rng, left), q, rand(rng, m - q.size - left)]).tobytes())
        else:
            left = int(rng.integers(0, q.size - m + 1))
            out.append(q[left:left + m].tobytes())
    return out


def rotated(refs, r):
    at = (r * (len(refs) // 7 + 1)) % max(len(refs), 1)
    return refs[at:] + refs[:at]


def hits_call(queries, refs, ks_q, ks_r, K, cov):
    """-> call(r) -> kernel ms on the database rotated r times; stats() of the last output"""
    jarr = calls.job_array([(0, len(queries), len(queries), len(refs))], _lib.HITS_JOB_DTYPE)
    keys = np.zeros(len(queries) * K, dtype=np.uint64)

    def call(r):
        order = rotated(list(range(len(refs))), r)
        seqs = list(queries) + [refs[i] for i in order]
        karr = calls.limits(list(ks_q) + [ks_r[i] for i in order])
        return device_ms("smx_best_hits", b"".join(seqs), _lib.ptr(calls.offsets(seqs)), len(seqs), _lib.ptr(karr), _lib.ptr(jarr), 1,
                         K, cov, _lib.ptr(keys))

    def stats():
        rows = keys.reshape(-1, K) != np.uint64(identify.NONE)
        return {"queries_with_hit": int(rows.any(axis=1).sum()), "slots_filled": int(rows.sum())}
    return call, stats


def mine_call(queries, refs, ks_q, min_identity):
    """smx_mine_best_identity over the same pairs: every query against every ref (the refs are the targets)."""
    qoff, karr = calls.offsets(queries), calls.limits(ks_q)
    jarr = calls.job_array([(0, len(queries), 0, len(refs), min_identity)], _lib.MINE_JOB_DTYPE)
    best = np.zeros(len(refs), dtype=np.float64)
    qblob = b"".join(queries)

    def call(r):
        rs = rotated(refs, r)
        return device_ms("smx_mine_best_identity", qblob, _lib.ptr(qoff), len(queries), _lib.ptr(karr), b"".join(rs),
                         _lib.ptr(calls.offsets(rs)), len(rs), _lib.ptr(jarr), 1, _lib.ptr(best))
    return call, lambda: {"targets_with_identity": int((best > 0).sum())}


def timed(calls, repeats):
    """Each call once as a warm-up, then `repeats` rounds that alternate between them, the database rotated every round."""
    ms = [[] for _ in calls]
    for r in range(repeats + 1):
        for i, call in enumerate(calls):
            t = call(r)
            if r:
                ms[i].append(t)
    return ms


def write_fasta(path, names, seqs):
    with open(path, "w") as fh:
        for n, s in zip(names, seqs):
            fh.write(f">{n}\n{s.decode()}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=768)
    ap.add_argument("--refs", type=int, default=100000)
    ap.add_argument("--length", type=int, default=650)
    ap.add_argument("--templates", type=int, default=96)
    ap.add_argument("--top", type=int, default=5)
    ap.add_argument("--min-coverage", type=float, default=0.5)
    ap.add_argument("--min-identity", type=float, default=0.90)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="A,B,C")
    ap.add_argument("--tool", action="store_true")
    a = ap.parse_args()
    import ctypes as C
    lib = _lib.load()
    _lib.check(lib.smx_device_init(0, C.byref(C.c_int(0))))
    rng = np.random.default_rng(1)
    cov = int(round(a.min_coverage * 1000))
    k_of = lambda s: specimine.max_distance(len(s), a.min_identity)   # noqa: E731
    queries = make_queries(rng, a.queries, a.length, a.templates)
    ks_q = [k_of(s) for s in queries]
    qmin, qmax = min(map(len, queries)), max(map(len, queries))
    base = {"bench": "best_hits", "queries": a.queries, "query_length": [qmin, qmax], "K": a.top, "min_cov_permille": cov,
            "min_identity": a.min_identity, "repeats": a.repeats}
    refs_a = None
    for shape in a.shapes.split(","):
        if shape == "A":
            refs = refs_a = make_refs(rng, queries, a.refs, max(qmax + 1, 700), max(qmax + 101, 800))
        elif shape == "B":
            refs = make_refs(rng, queries, a.refs, min(450, qmin - 101), min(550, qmin - 1))
        else:
            refs = list(queries)
        ks_r = [k_of(s) for s in refs]
        pairs = len(queries) * len(refs)
        h_call, h_stats = hits_call(queries, refs, ks_q, ks_r, a.top, cov)
        calls = [h_call]
        if shape == "A":
            m_call, m_stats = mine_call(queries, refs, ks_q, a.min_identity)
            calls.append(m_call)
        ms = timed(calls, a.repeats)
        line = dict(base, shape=shape, refs=len(refs), ref_length=[min(map(len, refs)), max(map(len, refs))], pairs=pairs,
                    **spread(ms[0]), pairs_per_s=round(pairs / (statistics.median(ms[0]) * 1e-3)), **h_stats())
        if shape == "A":
            line["mine_best_identity"] = dict(spread(ms[1]), pairs_per_s=round(pairs / (statistics.median(ms[1]) * 1e-3)), **m_stats())
            line["ratio_median"] = round(statistics.median(ms[0]) / statistics.median(ms[1]), 4)
            line["ratio_per_round"] = [round(x / y, 4) for x, y in zip(ms[0], ms[1])]
        print(json.dumps(line), flush=True)
    if a.tool:
        if refs_a is None:
            refs_a = make_refs(rng, queries, a.refs, max(qmax + 1, 700), max(qmax + 101, 800))
        with tempfile.TemporaryDirectory() as d:
            qf, df = os.path.join(d, "q.fasta"), os.path.join(d, "db.fasta")
            write_fasta(qf, [f"Q{i}" for i in range(len(queries))], queries)
            write_fasta(df, [f"R{i} synthetic ref {i}" for i in range(len(refs_a))], refs_a)
            args = identify.build_parser().parse_args(["--fasta", qf, "--db", df, "--strand", "plus", "--top", str(a.top),
                                                       "--min-coverage", str(a.min_coverage), "--min-identity", str(a.min_identity),
                                                       "--report", os.path.join(d, "r.tsv"), "--json", os.path.join(d, "r.json")])
            walls, kms = [], []
            for _ in range(3):
                ms, t0 = [], time.perf_counter()
                assert identify.run(args, kernel_ms=ms) == 0
                walls.append(round(time.perf_counter() - t0, 3))
                kms.append(round(sum(ms), 3))
            with open(os.path.join(d, "r.json")) as fh:
                summary = json.load(fh)["summary"]
        print(json.dumps({"bench": "identify_tool", "shape": "A", "strand": "plus", "wall_s": walls, "kernel_ms": kms,
                          "summary": summary}), flush=True)


if __name__ == "__main__":
    main()
