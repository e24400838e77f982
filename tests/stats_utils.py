"""Helpers of the specimux-stats tests (test_stats_cpu.py, test_stats_gpu.py): the oracle's trace as a stats table, and
the oracle's hit tables and primary records in the binary layout the statistics kernel reads (tests/cpu/stats_sim.cpp)."""
import json
import os
import types

import numpy as np

from oracle import specimux_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_GOLDEN = os.path.join(REPO, "tests", "golden", "stats")
QUERIES = json.load(open(os.path.join(STATS_GOLDEN, "queries.json")))
CASES = ["golden_default", "golden_n11_20", "golden_derep_none", "golden_no_preorient", "golden_min_length_600", "c2_synth"]


def queries_of(case):
    return [q for q in QUERIES if q["cases"] == "all" or case in q["cases"]]


def unpack_trace(case, tmp_path):
    """The case's trace.tsv.gz as a trace directory (one specimux_trace_*.tsv) under tmp_path."""
    import gzip
    d = tmp_path / f"trace_{case}"
    d.mkdir()
    with gzip.open(os.path.join(STATS_GOLDEN, case, "trace.tsv.gz"), "rb") as src:
        (d / "specimux_trace_fixture_main.tsv").write_bytes(src.read())
    return os.fspath(d)

# smx_hit / smx_op (include/smx.h), restated so that the CPU tests do not need the HIP library
HIT = np.dtype([("first_start", "<i4"), ("first_end", "<i4"), ("tail_end", "<i4"), ("pdist", "<i2"), ("nloc", "<i2"),
                ("bbest", "<i2"), ("ntied", "<i2"), ("first_tied", "<i2"), ("flags", "<i2")])
OP = np.dtype([("sample", "<i4"), ("trim_start", "<i4"), ("trim_end", "<i4"), ("pool", "<i2"), ("p1", "<i2"), ("p2", "<i2"),
               ("barcode", "<i2"), ("dist", "i1", (4,)), ("rtype", "u1"), ("flags", "u1"), ("n_ops", "<u2"), ("read", "<u4")])
OPF_TRIM_EMPTY = 2


def oracle_table(opanel, opar, reads):
    """(stats table the host aggregator builds from the oracle's level-1 trace of `reads`, the trace rows)."""
    from specimux_amd import trace_stats
    tr = O.Tracer(1, "main")
    ops, _t, _m = O.process_sequences(reads, opar, opanel, tr=tr, record_offset=1)
    O.trace_outputs(tr, ops)
    return trace_stats.table_from_rows(["t"] + row for row in tr.rows), tr.rows


def panel_view(opanel):
    """The index -> name tables of specimux_amd.panel.CompiledPanel (primer order, global barcode list, pair list with
    pools), built from the oracle's panel: what decode_key needs."""
    primers = list(opanel.primers.values())
    barcodes = []
    for p in primers:
        barcodes += [b for b in p.barcodes if b not in barcodes]
    pools, pairs = [], []
    pidx = {id(p): i for i, p in enumerate(primers)}
    for fp in opanel.get_primers(O.FWD):
        for rp in opanel.get_paired(fp.primer):
            pool = O.pool_from_primers(fp, rp)
            if pool is not None and pool not in pools:
                pools.append(pool)
            pairs.append((pidx[id(fp)], pidx[id(rp)], pools.index(pool) if pool is not None else -1))
    return types.SimpleNamespace(primers=primers, primer_names=[p.name for p in primers], barcodes=barcodes, pools=pools,
                                 pairs=pairs, pdir=[0 if p.direction == O.FWD else 1 for p in primers])


def sim_input(view, opanel, opar, reads):
    """Bytes of a stats_sim input: per read the oracle's search results as lean hit records and its primary record
    (rtype, n_ops, trim-empty flag) as the demux kernel would leave them.  Returns (bytes, ops, hits, per-barcode distances)."""
    NP = len(view.primers)
    prefilter = O.make_prefilter(opanel, opar) if opar.prefilter else None
    bidx = {b: i for i, b in enumerate(view.barcodes)}
    hits = np.zeros((len(reads), 2 * NP), dtype=HIT)
    bdist = np.full((len(reads), 2 * NP, max(len(p.barcodes) for p in view.primers)), -1, dtype=np.int8)
    ops = np.zeros(len(reads), dtype=OP)
    for i, rec in enumerate(reads):
        L = len(rec[1])
        ops["read"][i] = i
        if (opar.min_length != -1 and L < opar.min_length) or (opar.max_length != -1 and L > opar.max_length):
            continue   # rtype 0 = filtered
        table = O.hit_table(opar, opanel, rec, prefilter)
        s, rs = rec[1], O.revcomp(rec[1])
        for p, primer in enumerate(view.primers):
            k = opar.max_dist_primers[primer.primer]
            votes = (O.align_seq(primer.primer, s, k, 0, opar.search_len).matched(),
                     O.align_seq(primer.primer, rs, k, 0, opar.search_len).matched())
            for e, end in enumerate("AB"):
                h, t = hits[i, 2 * p + e], table[(primer.name, end)]
                h["pdist"], h["bbest"], h["first_tied"], h["flags"] = t["pdist"], -1, -1, int(votes[e])
                h["first_start"] = h["first_end"] = h["tail_end"] = -1
                if t["pdist"] >= 0:
                    h["nloc"], (h["first_start"], h["first_end"]) = len(t["locs"]), t["locs"][0]
                dists = {bc: d for bc, (d, _l) in t["barcodes"].items()}
                if t["pdist"] >= 0 and dists:
                    best = min(dists.values())
                    tied = [bc for bc in primer.barcodes if dists.get(bc) == best]
                    h["bbest"], h["ntied"], h["first_tied"] = best, len(tied), bidx[tied[0]]
                    h["tail_end"] = max(loc[1] for _d, locs in t["barcodes"].values() for loc in locs)
                    for bi, bc in enumerate(primer.barcodes):
                        bdist[i, 2 * p + e, bi] = dists.get(bc, -1)
        rops, _t, _m = O.process_sequences([rec], opar, opanel, prefilter)
        first = rops[0]
        ops["rtype"][i], ops["n_ops"][i] = first.rtype, len(rops)
        if (first.p1 == "unknown" and first.p1_loc is not None) or (first.p2 == "unknown" and first.p2_loc is not None):
            ops["flags"][i] |= OPF_TRIM_EMPTY    # the fallback record no longer names the primers its candidate matched
    head = np.array([NP, len(view.pairs), 1 if opar.preorient else 0, len(reads)], dtype="<i4")
    body = [head, np.array(view.pdir, dtype="<i4"), np.array([a for a, _b, _c in view.pairs], dtype="<i4"),
            np.array([b for _a, b, _c in view.pairs], dtype="<i4")]
    return b"".join(a.tobytes() for a in body) + hits.tobytes() + ops.tobytes(), ops, hits, bdist


def parse_sim(text):
    """stdout of stats_sim -> (counters dict, fallback read indices, {key: count})."""
    counters, fallback, keys = {}, [], {}
    for line in text.splitlines():
        w = line.split()
        if w[0] == "counters":
            counters = {k: int(v) for k, v in (x.split("=") for x in w[1:])}
        elif w[0] == "fallback":
            fallback.append(int(w[1]))
        elif w[0] == "key":
            keys[int(w[1], 16)] = int(w[2])
    return counters, fallback, keys
