#!/usr/bin/env python3
"""specimux-crosstalk: where did the foreign reads of a well come from?  (The reference has no such tool.)

Every read of every specimen file of a run (`full/<pool>/<S>.fastq`) is compared with every consensus sequence (ref) of
the run: the NW (global) edit distance, limited to max(k[ref], k[read]) with k = int(len * (1 - min_identity)).  All of
it happens on the GPU (smx_nearest, HIP kernel smx_nearest.hip), which returns per read two keys: the nearest ref of the
specimen the read is filed under (`own`) and the nearest ref of any other specimen (`other`), each as (distance, ref),
ties to the lower ref.  There is no CPU path.  The host then classes each read with integers only:

    unplaced    no ref within the limit
    own         an own ref, and no other ref nearer (ties are own)
    foreign     only another specimen's ref; or another specimen's ref nearer than the own one and the two refs at
                least `--min-separation` edits apart
    ambiguous   another specimen's ref nearer, but the two refs fewer than `--min-separation` edits apart: two wells
                with the same organism, where the read's own errors decide which is nearer

A source (A <- B) is flagged when at least `--min-reads` reads filed under A are foreign with a ref of specimen B; a
specimen is `no_reference` without a ref, `contaminated` with a flagged source, else `clean`.

    python -m specimux_amd.crosstalk --run-dir OUT [--level pool|primer-pair] (--consensus C.json | --refs R.fasta)
        [--min-identity 0.90] [--max-reads 0] [--min-separation 5] [--min-reads 5]
        [--report T.tsv] [--json J.json] [--reads READS.tsv]

Device calls are planned under clusters' byte budget (SMX_CLUSTERS_BUDGET_BYTES, else specimine's); a call costs the refs
plus its specimens' files, so the refs of a run must fit the budget.  One GPU."""
import argparse
import json
import logging
import os
import re
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import calls, clusters, consensus, specimine

NONE = 2**64 - 1                           # smx.h: a key without a ref
Key = Optional[Tuple[int, int]]            # (distance, ref index) or None
Job = Tuple[int, int, int, int]            # (q0, nq, t0, nt): indices into the call's sequence list
CLASSES = ("own", "ambiguous", "unplaced", "foreign")


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Trace every read of a run to the nearest consensus sequence of the run.")
    parser.add_argument("--run-dir", required=True, help="specimux output directory: every specimen file under RUN_DIR/full/")
    parser.add_argument("--level", choices=("pool", "primer-pair"), default="pool",
                        help="full/<pool>/<S>.fastq (pool) or full/<pool>/<pair>/<S>.fastq (default: pool)")
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("--consensus", help="The --json file of specimux-consensus over the same run: the refs, each with "
                                            "its specimen's file")
    source.add_argument("--refs", help="A FASTA file of refs; a record belongs to the specimen whose id equals its name up "
                                       "to the first blank, a trailing _c<digits> removed (specimux-consensus --fasta)")
    parser.add_argument("--min-identity", type=float, default=0.90,
                        help="A read is compared with a ref up to int(len * (1 - this)) edits of the longer limit, as in "
                             "specimux-clusters (default: 0.90)")
    parser.add_argument("--max-reads", type=int, default=0,
                        help="Use at most this many reads per specimen, the best by mean quality; 0: all (default: 0)")
    parser.add_argument("--min-separation", type=int, default=5,
                        help="A read nearer to another specimen's ref than to its own is foreign only if the two refs are "
                             "at least this many edits apart, else ambiguous.  A choice of the user's, like "
                             "--min-identity, not a measured constant (default: 5)")
    parser.add_argument("--min-reads", type=int, default=5,
                        help="Foreign reads from one source specimen that flag the source.  A choice of the user's, not a "
                             "measured constant (default: 5)")
    parser.add_argument("--report", help="Write a TSV: one row per specimen, then one row per flagged source")
    parser.add_argument("--json", help="Write the same content as JSON, with the run summary")
    parser.add_argument("--reads", help="Write a TSV with one row per read: its class and its two nearest refs")
    parser.add_argument("--debug", action="store_true", help="Enable debug logging")
    return parser


# ------------------------------------------------------------------------------------------------ refs
class Ref:
    """One consensus sequence: its record name, the specimen it belongs to (a name, and the index of the specimen's file
    among the run's files or None) and its sequence."""
    __slots__ = ("name", "specimen", "file", "seq")

    def __init__(self, name: str, specimen: str, file: Optional[int], seq: str):
        self.name, self.specimen, self.file, self.seq = name, specimen, file, seq


def refs_from_consensus(path: str, files: Sequence[str]) -> List[Ref]:
    """The refs of a specimux-consensus --json file, in file order; a specimen is matched to the run's files by path."""
    with open(path, "r", encoding="latin-1") as fh:
        doc = json.load(fh)
    index = {os.path.abspath(f): i for i, f in enumerate(files)}
    out = []
    for spec in doc.get("specimens", []):
        at = index.get(os.path.abspath(spec["specimen"]))
        try:
            name = specimine.extract_specimen_id(spec["specimen"])
        except ValueError:
            name = os.path.basename(spec["specimen"])
        for c in spec.get("clusters", []):
            if c.get("consensus"):
                out.append(Ref(c["name"], name, at, c["consensus"]))
    return out


def ref_specimen_name(record_name: str) -> str:
    """The specimen id a FASTA record name stands for: the name up to the first blank, a trailing _c<digits> removed."""
    words = record_name.split()
    return re.sub(r"_c\d+$", "", words[0]) if words else ""


def refs_from_fasta(path: str, files: Sequence[str]) -> List[Ref]:
    """The refs of a FASTA file, in file order.  A name that matches the files of two pools is an error naming both."""
    by_id: Dict[str, List[int]] = {}
    for i, f in enumerate(files):
        by_id.setdefault(specimine.extract_specimen_id(f), []).append(i)
    out: List[Ref] = []
    name, chunks = None, []

    def flush():
        if name is None:
            return
        words = name.split()
        spec = ref_specimen_name(name)
        hits = by_id.get(spec, [])
        if len(hits) > 1:
            raise ValueError(f"ref {words[0] if words else ''!r}: specimen {spec!r} matches {files[hits[0]]} and "
                             f"{files[hits[1]]}; use --consensus, which carries the file of each specimen")
        seq = "".join(chunks)
        if seq:
            out.append(Ref(words[0] if words else "", spec, hits[0] if hits else None, seq))

    with open(path, "r", encoding="latin-1") as fh:
        for line in fh:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                flush()
                name, chunks = line[1:], []
            elif name is not None:
                chunks.append(line.strip())
    flush()
    return out


def ref_groups(refs: Sequence[Ref], n_files: int) -> List[int]:
    """The group of each ref: its specimen's file index; refs that match no file get a group per specimen name behind."""
    extra: Dict[str, int] = {}
    return [r.file if r.file is not None else extra.setdefault(r.specimen, n_files + len(extra)) for r in refs]


# ------------------------------------------------------------------------------------------------ the device call
nearest = calls.nearest
nearest_distances = calls.nearest_distances


def reduce_distances(dist: np.ndarray, q0: int, ref_groups_: Sequence[int], read_groups: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """The two keys of every read of one job from its nq x nt distances: the host twin of the kernel's reduction."""
    nq, nt = dist.shape
    own = np.full(nt, NONE, dtype=np.uint64)
    other = np.full(nt, NONE, dtype=np.uint64)
    for t in range(nt):
        for q in range(nq):
            d = int(dist[q, t])
            if d < 0:
                continue
            key = (d << 32) | (q0 + q)
            side = own if ref_groups_[q] == read_groups[t] else other
            if key < int(side[t]):
                side[t] = key
    return own, other


def nearest_oracle(seqs: Sequence[bytes], ks: Sequence[int], groups: Sequence[int], jobs: Sequence[Job],
                   kernel_ms: Optional[list] = None) -> Tuple[np.ndarray, np.ndarray]:
    """nearest() by the suite's oracle (edlib NW semantics, exact byte equality), pair by pair on the CPU.  For tests."""
    from oracle.edlib_semantics import NW, align_c
    texts = [s.decode("latin-1") for s in seqs]
    owns, others = [], []
    for q0, nq, t0, nt in jobs:
        dist = np.full((nq, nt), -1, dtype=np.int64)
        for q in range(nq):
            for t in range(nt):
                kq, kt = ks[q0 + q], ks[t0 + t]
                k = -1 if kq < 0 or kt < 0 else max(kq, kt)
                if texts[t0 + t]:
                    dist[q, t] = align_c(texts[q0 + q], texts[t0 + t], NW, k, iupac=False)["editDistance"]
                else:                                  # an empty read costs the ref's length
                    dist[q, t] = len(texts[q0 + q]) if k < 0 or len(texts[q0 + q]) <= k else -1
        o, x = reduce_distances(dist, q0, groups[q0:q0 + nq], groups[t0:t0 + nt])
        owns.append(o)
        others.append(x)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)   # noqa: E731
    return cat(owns), cat(others)


def decode(key: int) -> Key:
    key = int(key)
    return None if key == NONE else (key >> 32, key & 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the class rule
def classify(own: Key, oth: Key, ref_distance: Callable[[int, int], int], min_separation: int) -> str:
    """The class of one read from its two decoded keys.  ref_distance(a, b) is the NW distance of refs a and b; it is
    asked only when both keys exist and the other ref is strictly nearer."""
    if own is None and oth is None:
        return "unplaced"
    if oth is None or (own is not None and own[0] <= oth[0]):
        return "own"
    if own is None:
        return "foreign"
    return "foreign" if ref_distance(own[1], oth[1]) >= min_separation else "ambiguous"


class RefDistances:
    """NW distances between refs (consensus.nw_distance), computed once per distinct pair."""
    def __init__(self, refs: Sequence[Ref]):
        self.refs = refs
        self.cache: Dict[Tuple[int, int], int] = {}

    def __call__(self, a: int, b: int) -> int:
        key = (min(a, b), max(a, b))
        if key not in self.cache:
            self.cache[key] = consensus.nw_distance(self.refs[key[0]].seq, self.refs[key[1]].seq) if a != b else 0
        return self.cache[key]


# ------------------------------------------------------------------------------------------------ one run
class ReadResult:
    __slots__ = ("id", "cls", "own", "oth")

    def __init__(self, id: str, cls: str, own: Key, oth: Key):
        self.id, self.cls, self.own, self.oth = id, cls, own, oth


class SpecimenResult:
    def __init__(self, index: int, path: str, n_records: int):
        self.index, self.path, self.n_records = index, path, n_records
        self.reads: List[ReadResult] = []
        self.refs: List[int] = []              # the specimen's refs, in ref order (the first is its rank-1 ref)
        self.status = "clean"
        self.sources: List[Dict] = []          # the flagged sources

    def counts(self) -> Dict[str, int]:
        c = {k: 0 for k in CLASSES}
        for r in self.reads:
            c[r.cls] += 1
        return c


def flag_sources(res: SpecimenResult, refs: Sequence[Ref], groups: Sequence[int], files: Sequence[str],
                 ref_distance: Callable[[int, int], int], min_reads: int) -> List[Dict]:
    """The flagged sources of one specimen: per source specimen with >= min_reads foreign reads its name (the file where
    it has one), the ref most of those reads are nearest to (ties: the lower ref), the reads, their share of the
    specimen's reads, the smallest and the (lower) median distance, and the distance of that ref to the specimen's
    rank-1 ref.  Most reads first, then the lower source group."""
    by_group: Dict[int, List[ReadResult]] = {}
    for r in res.reads:
        if r.cls == "foreign":
            by_group.setdefault(groups[r.oth[1]], []).append(r)
    out = []
    for g, rs in sorted(by_group.items(), key=lambda kv: (-len(kv[1]), kv[0])):
        if len(rs) < min_reads:
            continue
        per_ref: Dict[int, int] = {}
        for r in rs:
            per_ref[r.oth[1]] = per_ref.get(r.oth[1], 0) + 1
        top = min(per_ref, key=lambda q: (-per_ref[q], q))
        ds = sorted(r.oth[0] for r in rs)
        out.append({"source": files[g] if g < len(files) else refs[top].specimen, "source_ref": refs[top].name,
                    "reads": len(rs), "share": round(len(rs) / len(res.reads), 4), "min_distance": ds[0],
                    "median_distance": ds[(len(ds) - 1) // 2],
                    "ref_distance": ref_distance(top, res.refs[0]) if res.refs else None})
    return out


def crosstalk_files(paths: Sequence[str], refs: Sequence[Ref], min_identity: float = 0.90, max_reads: int = 0,
                    min_separation: int = 5, min_reads: int = 5, budget: Optional[int] = None,
                    nearest_fn: Callable = nearest, kernel_ms: Optional[list] = None) -> Tuple[List[SpecimenResult], Dict]:
    """Class every read of every file of `paths` that can be read against `refs`.  Returns the results in the order of
    `paths` and the run summary."""
    budget = budget if budget is not None else clusters.budget_bytes()
    groups = ref_groups(refs, len(paths))
    ref_seqs = [r.seq.encode("latin-1") for r in refs]
    ref_ks = [specimine.max_distance(len(r.seq), min_identity) for r in refs]
    ref_bytes = sum(len(s) for s in ref_seqs)
    ref_distance = RefDistances(refs)
    sizes = []
    for p in paths:
        try:
            sizes.append(os.path.getsize(p))
        except OSError:
            sizes.append(0)
    results: List[Optional[SpecimenResult]] = [None] * len(paths)
    summary = {"specimens": len(paths), "read": 0, "failed": 0, "refs": len(refs), "reads": 0, "placed": 0, "foreign": 0,
               "foreign_share": 0.0, "flagged_sources": 0, "contaminated": 0, "device_calls": 0}
    # a call costs the refs, once, plus its specimens' files
    for call in specimine.plan_calls([(s, [("refs", ref_bytes)]) for s in sizes], budget):
        batch: List[Tuple[SpecimenResult, List[clusters.Read]]] = []
        for i in sorted(call):
            try:
                records = clusters.read_records(paths[i])
            except (OSError, ValueError) as e:
                logging.error(f"Could not read {paths[i]}: {e}")
                summary["failed"] += 1
                continue
            keep = clusters.sample_top_quality([r.qual for r in records], max_reads) if max_reads > 0 else range(len(records))
            batch.append((SpecimenResult(i, paths[i], len(records)), [records[x] for x in keep]))
        seqs, ks, grp, jobs = list(ref_seqs), list(ref_ks), list(groups), []
        for res, recs in batch:
            jobs.append((0, len(refs), len(seqs), len(recs)))
            for r in recs:
                seqs.append(r.seq.encode("latin-1"))
                ks.append(specimine.max_distance(len(r.seq), min_identity))
                grp.append(res.index)
        if any(j[3] for j in jobs):
            own, other = nearest_fn(seqs, ks, grp, jobs, kernel_ms)
            summary["device_calls"] += 1
        else:
            own = other = np.zeros(0, dtype=np.uint64)
        at = 0
        for res, recs in batch:
            for r in recs:
                o, x = decode(own[at]), decode(other[at])
                res.reads.append(ReadResult(r.id, classify(o, x, ref_distance, min_separation), o, x))
                at += 1
            res.refs = [q for q, g in enumerate(groups) if g == res.index]
            res.sources = flag_sources(res, refs, groups, paths, ref_distance, min_reads)
            res.status = "no_reference" if not res.refs else "contaminated" if res.sources else "clean"
            c = res.counts()
            summary["read"] += 1
            summary["reads"] += len(res.reads)
            summary["placed"] += len(res.reads) - c["unplaced"]
            summary["foreign"] += c["foreign"]
            summary["flagged_sources"] += len(res.sources)
            summary["contaminated"] += res.status == "contaminated"
            results[res.index] = res
    summary["foreign_share"] = round(summary["foreign"] / summary["placed"], 4) if summary["placed"] else 0.0
    return [r for r in results if r is not None], summary


# ------------------------------------------------------------------------------------------------ outputs
COLUMNS = ("specimen", "status", "reads", "own", "ambiguous", "unplaced", "foreign", "refs")
SOURCE_COLUMNS = ("specimen", "source", "source_ref", "reads", "share", "min_distance", "median_distance", "ref_distance")
READ_COLUMNS = ("specimen", "read", "class", "own_ref", "own_distance", "other_ref", "other_distance")


def tsv_text(results: Sequence[SpecimenResult]) -> str:
    lines = ["\t".join(COLUMNS)]
    for res in results:
        c = res.counts()
        lines.append("\t".join(str(x) for x in (res.path, res.status, len(res.reads), c["own"], c["ambiguous"], c["unplaced"],
                                                c["foreign"], len(res.refs))))
    lines.append("")
    lines.append("\t".join(SOURCE_COLUMNS))
    for res in results:
        for s in res.sources:
            lines.append("\t".join(str(x) for x in (res.path, s["source"], s["source_ref"], s["reads"], f"{s['share']:.4f}",
                                                    s["min_distance"], s["median_distance"],
                                                    "-" if s["ref_distance"] is None else s["ref_distance"])))
    return "\n".join(lines) + "\n"


def json_text(results: Sequence[SpecimenResult], summary: Dict) -> str:
    return json.dumps({"summary": summary,
                       "specimens": [dict({"specimen": res.path, "status": res.status, "reads": len(res.reads)}, **res.counts(),
                                          refs=len(res.refs), sources=res.sources) for res in results]}, indent=1) + "\n"


def reads_text(results: Sequence[SpecimenResult], refs: Sequence[Ref]) -> str:
    lines = ["\t".join(READ_COLUMNS)]
    for res in results:
        for r in res.reads:
            cols = [res.path, r.id, r.cls]
            for key in (r.own, r.oth):
                cols += ["-", "-"] if key is None else [refs[key[1]].name, str(key[0])]
            lines.append("\t".join(cols))
    return "\n".join(lines) + "\n"


def summary_line(summary: Dict) -> str:
    return (f"Traced {summary['reads']} read(s) of {summary['read']} of {summary['specimens']} specimen(s) to {summary['refs']} "
            f"ref(s) in {summary['device_calls']} device call(s): {summary['placed']} placed, {summary['foreign']} foreign "
            f"({summary['foreign_share']:.4f} of the placed); {summary['flagged_sources']} source(s) flagged, "
            f"{summary['contaminated']} specimen(s) contaminated")


def run(args, nearest_fn: Callable = nearest, kernel_ms: Optional[list] = None) -> int:
    """Everything main() does after parsing; returns the exit status (1 only if no file could be read)."""
    paths = specimine.discover_specimens(args.run_dir, args.level)
    refs = refs_from_consensus(args.consensus, paths) if args.consensus else refs_from_fasta(args.refs, paths)
    results, summary = crosstalk_files(paths, refs, args.min_identity, args.max_reads, args.min_separation, args.min_reads,
                                       nearest_fn=nearest_fn, kernel_ms=kernel_ms)
    if summary["read"] == 0:
        logging.error("No specimen file could be read")
        return 1
    for res in results:
        for s in res.sources:
            logging.info(f"flagged: {res.path} <- {s['source']}: {s['reads']} read(s) nearest to {s['source_ref']}")
    logging.info(summary_line(summary))
    specimine.write_texts(((args.report, lambda: tsv_text(results)), (args.json, lambda: json_text(results, summary)),
                           (args.reads, lambda: reads_text(results, refs))))
    return 0


def main(argv=None):
    specimine.tool_main(build_parser, run, argv, value_error_status=2)


if __name__ == "__main__":
    main()
