#!/usr/bin/env python3
"""specimux-clusters throughput on a synthetic run: S specimens x R reads of ~L nt with 2 % per-read error, two
templates (the second a 25 % mutation of the first, 30 % of the reads) in a tenth of the specimens.  Prints JSON lines:

  pairs_all      smx_pairs_neighbours over every specimen in one call: kernel ms (HIP events; min / median / max over
                 the repeats after one warm-up call) and pairs/s
  yardstick      the same --yard-specimens specimens through smx_pairs_distances, smx_pairs_neighbours and
                 smx_mine_distances (queries = targets = the specimen's reads, the same per-read k; n^2 pairs per
                 specimen against n (n - 1) / 2), each with its rate per pair (the three calls alternate), and the
                 ratio pairs / mine; once more for one specimen alone (a grid that does not fill the device)
  run_dir        end-to-end seconds of `--run-dir` (reading, sampling, device calls, clustering, report) and what it found

    python tools/cluster_bench.py [--specimens 96 --reads 500 --length 650 --min-identity 0.90 --repeats 5]"""
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

from specimux_amd import _lib, calls, clusters, specimine  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def mutate(rng, s, rate):
    """The suite's mutation model on a uint8 array: per base a substitution, an insertion behind it or a deletion,
    each with probability rate / 3."""
    r = rng.random(s.size)
    count = np.where(r < rate / 3, 1, np.where(r < 2 * rate / 3, 2, np.where(r < rate, 0, 1)))
    out = np.repeat(s, count)
    first = np.cumsum(count) - count
    sub = first[r < rate / 3]
    out[sub] = BASES[rng.integers(0, 4, sub.size)]
    ins = first[(r >= rate / 3) & (r < 2 * rate / 3)] + 1
    out[ins] = BASES[rng.integers(0, 4, ins.size)]
    return out


def write_tree(root, specimens, reads, length, error, seed=1):
    rng = np.random.default_rng(seed)
    pool = os.path.join(root, "full", "POOL")
    os.makedirs(pool, exist_ok=True)
    mixed = 0
    for s in range(specimens):
        t1 = BASES[rng.integers(0, 4, int(length * rng.uniform(0.95, 1.05)))]
        two = s % 10 == 0
        mixed += two
        t2 = mutate(rng, t1, 0.25)
        with open(os.path.join(pool, f"S{s:03d}.fastq"), "wb") as fh:
            for i in range(reads):
                seq = mutate(rng, t2 if two and i % 10 < 3 else t1, error)
                qual = (33 + rng.integers(10, 41, seq.size)).astype(np.uint8)
                fh.write(b"@S%03d_%d\n%s\n+\n%s\n" % (s, i, seq.tobytes(), qual.tobytes()))
    return mixed


def spread(ms):
    return {"kernel_ms_min": round(min(ms), 3), "kernel_ms_median": round(statistics.median(ms), 3),
            "kernel_ms_max": round(max(ms), 3)}


def device_ms(name, *args):
    """One libsmx call through calls.invoke -> the device time it reports."""
    ms = []
    calls.invoke(name, *args, kernel_ms=ms)
    return ms[0]


def pairs_call(specimens, neighbours):
    """-> (call() -> kernel ms, within() -> pairs within their limit in the last output)"""
    reads = [r for rs, _ in specimens for r in rs]
    roff = calls.offsets(reads)
    karr = calls.limits([k for _, ks in specimens for k in ks])
    jobs, at = [], 0
    for rs, _ in specimens:
        jobs.append((at, len(rs)))
        at += len(rs)
    jobs = calls.job_array(jobs, _lib.PAIRS_JOB_DTYPE)
    n_out = sum(len(rs) * ((len(rs) + 31) // 32) if neighbours else len(rs) * (len(rs) - 1) // 2 for rs, _ in specimens)
    out = np.zeros(max(n_out, 1), dtype=np.uint32 if neighbours else np.int32)
    name = "smx_pairs_neighbours" if neighbours else "smx_pairs_distances"
    blob = b"".join(reads)

    def call():
        return device_ms(name, blob, _lib.ptr(roff), len(reads), _lib.ptr(karr), _lib.ptr(jobs), len(specimens), _lib.ptr(out))

    return call, lambda: int(np.unpackbits(out.view(np.uint8)).sum()) // 2 if neighbours else int((out >= 0).sum())


def mine_call(specimens):
    reads = [r for rs, _ in specimens for r in rs]
    off = calls.offsets(reads)
    karr = calls.limits([k for _, ks in specimens for k in ks])
    jobs, at = [], 0
    for rs, _ in specimens:
        jobs.append((at, len(rs), at, len(rs), 0.0))
        at += len(rs)
    jarr = calls.job_array(jobs, _lib.MINE_JOB_DTYPE)
    out = np.zeros(sum(len(rs) ** 2 for rs, _ in specimens), dtype=np.int32)
    blob = b"".join(reads)

    def call():
        return device_ms("smx_mine_distances", blob, _lib.ptr(off), len(reads), _lib.ptr(karr), blob, _lib.ptr(off), len(reads),
                         _lib.ptr(jarr), len(jobs), _lib.ptr(out))

    return call, lambda: int((out >= 0).sum())


def timed(fns, repeats):
    """Each call once as a warm-up, then `repeats` rounds that alternate between them.  -> kernel ms per call."""
    ms = [[] for _ in fns]
    for r in range(repeats + 1):
        for i, call in enumerate(fns):
            t = call()
            if r:
                ms[i].append(t)
    return ms


def yardstick(specimens, repeats):
    tri = clusters.pair_count(specimens)
    square = sum(len(rs) ** 2 for rs, _ in specimens)
    (d_call, d_in), (n_call, n_in) = pairs_call(specimens, False), pairs_call(specimens, True)
    m_call, m_in = mine_call(specimens)
    d_ms, n_ms, m_ms = timed([d_call, n_call, m_call], repeats)
    d_within, n_within, m_within = d_in(), n_in(), m_in()
    rate = lambda pairs, ms: pairs / (statistics.median(ms) / 1e3)   # noqa: E731
    return {"bench": "yardstick", "specimens": len(specimens),
            "pairs_distances": dict(spread(d_ms), pairs=tri, pairs_per_s=round(rate(tri, d_ms), 1), within_limit=d_within),
            "pairs_neighbours": dict(spread(n_ms), pairs=tri, pairs_per_s=round(rate(tri, n_ms), 1), within_limit=n_within),
            "mine_distances": dict(spread(m_ms), pairs=square, pairs_per_s=round(rate(square, m_ms), 1), within_limit=m_within),
            "pairs_over_mine_rate": round(rate(tri, d_ms) / rate(square, m_ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--specimens", type=int, default=96)
    ap.add_argument("--reads", type=int, default=500)
    ap.add_argument("--length", type=int, default=650)
    ap.add_argument("--error", type=float, default=0.02)
    ap.add_argument("--min-identity", type=float, default=0.90)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--yard-specimens", type=int, default=16)
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    import ctypes as C
    lib = _lib.load()
    _lib.check(lib.smx_device_init(0, C.byref(C.c_int(0))))
    root = a.workdir or tempfile.mkdtemp(prefix="cluster_bench_")
    t0 = time.perf_counter()
    n_two = write_tree(root, a.specimens, a.reads, a.length, a.error)
    gen_s = time.perf_counter() - t0
    paths = specimine.discover_specimens(root, "pool")
    specimens = []
    for p in paths:
        recs = clusters.read_records(p)
        specimens.append(([r.seq.encode("latin-1") for r in recs],
                          [specimine.max_distance(len(r.seq), a.min_identity) for r in recs]))
    shape = {"specimens": a.specimens, "reads_per_specimen": a.reads, "read_length": a.length, "error": a.error,
             "min_identity": a.min_identity, "two_template_specimens": n_two, "repeats": a.repeats,
             "tree_generation_s": round(gen_s, 1)}
    call, count = pairs_call(specimens, True)
    ms, within = timed([call], a.repeats)[0], count()
    pairs = clusters.pair_count(specimens)
    print(json.dumps(dict({"bench": "pairs_all"}, **shape, pairs=pairs, within_limit=within, **spread(ms),
                          pairs_per_s=round(pairs / (statistics.median(ms) / 1e3), 1))), flush=True)
    print(json.dumps(yardstick(specimens[:a.yard_specimens], a.repeats)), flush=True)
    print(json.dumps(yardstick(specimens[1:2], a.repeats)), flush=True)
    e2e, kms = [], []
    args = clusters.build_parser().parse_args(["--run-dir", root, "--min-identity", repr(a.min_identity), "--max-reads",
                                               str(a.reads), "--report", os.path.join(root, "report.tsv")])
    for _ in range(3):
        k = []
        t0 = time.perf_counter()
        status = clusters.run(args, kernel_ms=k)
        e2e.append(time.perf_counter() - t0)
        kms.append(sum(k))
    with open(os.path.join(root, "report.tsv")) as fh:
        rows = [ln.split("\t") for ln in fh.read().splitlines()[1:]]
    print(json.dumps({"bench": "run_dir", "status": status, "e2e_s_min": round(min(e2e), 3),
                      "e2e_s_median": round(statistics.median(e2e), 3), "e2e_s_max": round(max(e2e), 3),
                      "kernel_ms_median": round(statistics.median(kms), 3),
                      "mixed_specimens": len({r[0] for r in rows if r[3] == "mixed"}),
                      "expected_mixed": n_two, "report_rows": len(rows)}), flush=True)


if __name__ == "__main__":
    main()
