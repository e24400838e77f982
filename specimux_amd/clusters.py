#!/usr/bin/env python3
"""specimux-clusters: is a demultiplexed specimen one sequence, or is the well mixed?  (The reference has no such
tool: the question is left to the clustering step after it.)

For each specimen file (`full/<pool>/<S>.fastq`) the reads -- the `--max-reads` best by mean Phred quality if there
are more -- are compared all against all: the NW (global) edit distance of reads i and j, limited to
max(k[i], k[j]) with k[i] = int(len_i * (1 - min_identity)).  Every distance is computed on the GPU
(smx_pairs_neighbours, HIP kernel smx_pairs.hip), which returns one adjacency bit per pair; there is no CPU path.  The
host then clusters greedily: the unassigned read with the most unassigned neighbours (ties: higher mean quality, then
lower file index) becomes a centre and takes those neighbours, until no read is left.  Cluster sizes come out
non-increasing.  A specimen is `mixed` if its second cluster has at least `--min-cluster-size` reads and at least
`--minor-share` of the sampled reads.

    python -m specimux_amd.clusters --fastq full/POOL/SPECIMEN.fastq [--report R.tsv] [--json R.json]
        [--centres C.fasta] [--split DIR] [--min-identity 0.90] [--max-reads 500] [--min-cluster-size 5]
        [--minor-share 0.10]
    python -m specimux_amd.clusters --run-dir OUT [--level pool|primer-pair] [...]

`--run-dir` takes every specimen file under OUT/full/ (specimine.discover_specimens) in device calls planned under a
byte budget (SMX_CLUSTERS_BUDGET_BYTES, else specimine's SMX_MINE_BUDGET_BYTES).  One GPU."""
import argparse
import json
import logging
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import calls, specimine

Specimen = Tuple[List[bytes], List[int]]   # one specimen's sampled reads and their limits k


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Find specimens whose reads hold two sequences.")
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("--fastq", help="Path to one specimen's FASTQ file")
    source.add_argument("--run-dir", help="specimux output directory: every specimen file under RUN_DIR/full/")
    parser.add_argument("--level", choices=("pool", "primer-pair"), default="pool",
                        help="--run-dir: full/<pool>/<S>.fastq (pool) or full/<pool>/<pair>/<S>.fastq (default: pool)")
    parser.add_argument("--min-identity", type=float, default=0.90,
                        help="Two reads are neighbours if their global edit distance is at most int(len * (1 - this)) of "
                             "the longer limit.  Global distance counts every overhang, so this suits reads trimmed to "
                             "barcodes or primers (--trim barcodes / primers); lower it for untrimmed reads "
                             "(default: 0.90)")
    parser.add_argument("--max-reads", type=int, default=500,
                        help="Compare at most this many reads per specimen, the best by mean quality (default: 500)")
    parser.add_argument("--min-cluster-size", type=int, default=5,
                        help="Smallest second cluster that makes a specimen mixed, and smallest cluster written to "
                             "--centres / --split (default: 5)")
    parser.add_argument("--minor-share", type=float, default=0.10,
                        help="Smallest share of the sampled reads in the second cluster that makes a specimen mixed "
                             "(default: 0.10)")
    parser.add_argument("--report", help="Write a TSV with one row per specimen and cluster")
    parser.add_argument("--json", help="Write the same content as JSON")
    parser.add_argument("--centres", help="Write the centre read of every cluster of >= --min-cluster-size reads (FASTA)")
    parser.add_argument("--split", help="Write DIR/<path below full/>/<S>.c<rank>.fastq for those clusters")
    parser.add_argument("--debug", action="store_true", help="Enable debug logging")
    return parser


# ------------------------------------------------------------------------------------------------ reading and sampling
class Read:
    """One FASTQ record: its id, sequence and quality (one character per byte) and its bytes in the file."""
    __slots__ = ("id", "seq", "qual", "raw")

    def __init__(self, id: str, seq: str, qual: str, raw: bytes):
        self.id, self.seq, self.qual, self.raw = id, seq, qual, raw


def read_records(path: str) -> List[Read]:
    """The records of a FASTQ file with io_utils.parse_fastq's tolerance (wrapped lines, '@' as a first quality
    character), each with the exact bytes it occupies in the file."""
    with open(path, "rb") as fh:
        lines = fh.read().splitlines(keepends=True)
    out: List[Read] = []
    i, n = 0, len(lines)
    while i < n:
        if not lines[i].strip():
            i += 1
            continue
        if lines[i][:1] != b"@":
            raise ValueError("Records in Fastq files should start with '@' character")
        start = i
        title = lines[i][1:].rstrip(b"\r\n").decode("latin-1")
        i += 1
        seq = b""
        while i < n and lines[i][:1] != b"+":
            seq += lines[i].strip()
            i += 1
        if i >= n:
            raise ValueError("End of file without quality information.")
        i += 1
        qual = b""
        if i < n:
            qual = lines[i].strip()
            i += 1
        while i < n and not (lines[i][:1] == b"@" and len(qual) >= len(seq)):
            qual += lines[i].strip()
            i += 1
        if len(qual) != len(seq):
            raise ValueError(f"Lengths of sequence and quality values differs for {title} ({len(seq)} and {len(qual)}).")
        words = title.split(None, 1)
        out.append(Read(words[0] if words else "", seq.decode("latin-1"), qual.decode("latin-1"), b"".join(lines[start:i])))
    return out


def mean_quality(qual: str) -> float:
    """orchestration.subsample_top_quality's key: the mean Phred quality of a record, 0 without quality."""
    return (sum(map(ord, qual)) / len(qual) - 33) if qual else 0


def sample_top_quality(quals: Sequence[str], max_reads: int) -> List[int]:
    """The indices of the max_reads records of highest mean quality, in file order: the records
    orchestration.subsample_top_quality keeps (a stable sort, so the earlier of two equal records wins)."""
    order = sorted(range(len(quals)), key=lambda i: mean_quality(quals[i]), reverse=True)
    return sorted(order[:max(max_reads, 0)])


# ------------------------------------------------------------------------------------------------ adjacency
def pair_count(specimens: Sequence[Specimen]) -> int:
    return sum(len(r) * (len(r) - 1) // 2 for r, _ in specimens)


def adjacency(specimens: Sequence[Specimen], kernel_ms: Optional[list] = None) -> List[np.ndarray]:
    """One smx_pairs_neighbours call: per specimen the symmetric boolean n x n matrix "NW distance of reads i and j
    <= max(k[i], k[j])", with a false diagonal."""
    jobs, at = [], 0
    for rs, _ in specimens:
        jobs.append((at, len(rs)))
        at += len(rs)
    words = calls.pairs_neighbours([r for rs, _ in specimens for r in rs], [k for _, ks in specimens for k in ks], jobs, kernel_ms)
    return [np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :len(rows)].astype(bool) if len(rows)
            else np.zeros((0, 0), dtype=bool) for rows in words]


def adjacency_oracle(specimens: Sequence[Specimen], kernel_ms: Optional[list] = None) -> List[np.ndarray]:
    """adjacency() by the suite's oracle (edlib NW semantics, exact byte equality), pair by pair on the CPU.  For tests."""
    from oracle.edlib_semantics import NW, align_c
    out = []
    for rs, ks in specimens:
        n = len(rs)
        texts = [r.decode("latin-1") for r in rs]
        a = np.zeros((n, n), dtype=bool)
        for i in range(n):
            for j in range(i + 1, n):
                k = -1 if ks[i] < 0 or ks[j] < 0 else max(ks[i], ks[j])
                a[i, j] = a[j, i] = align_c(texts[i], texts[j], NW, k, iupac=False)["editDistance"] >= 0
        out.append(a)
    return out


# ------------------------------------------------------------------------------------------------ clustering
def star_clusters(adj: np.ndarray, quality: Sequence[float]) -> List[List[int]]:
    """Greedy star clustering of the graph `adj` (symmetric, boolean, false diagonal).  Until no read is unassigned: the
    centre is the unassigned read with the most unassigned neighbours (ties: higher quality, then lower index); its
    cluster is the centre, listed first, and those neighbours in index order.  Sizes are non-increasing: taking
    reads away only lowers the degrees that are left."""
    n = adj.shape[0]
    free = np.ones(n, dtype=bool)
    deg = adj.sum(axis=1).astype(np.int64)
    q = np.asarray(quality, dtype=np.float64)
    clusters: List[List[int]] = []
    while free.any():
        cand = np.nonzero(free)[0]
        best = deg[cand].max()
        cand = cand[deg[cand] == best]
        if cand.size > 1:
            cand = cand[q[cand] == q[cand].max()]
        centre = int(cand[0])
        members = np.nonzero(adj[centre] & free)[0]
        taken = np.concatenate(([centre], members))
        free[taken] = False
        deg -= adj[:, taken].sum(axis=1)
        clusters.append([centre] + [int(m) for m in members])
    return clusters


def status_of(sizes: Sequence[int], sampled: int, min_cluster_size: int, minor_share: float) -> str:
    """`mixed` if the second cluster has >= min_cluster_size reads and its share (size / sampled, the figure the report
    shows) is >= minor_share."""
    if len(sizes) >= 2 and sizes[1] >= min_cluster_size and sizes[1] / sampled >= minor_share:
        return "mixed"
    return "ok"


# ------------------------------------------------------------------------------------------------ one run
class SpecimenResult:
    def __init__(self, path: str, records: List[Read], sampled: List[int]):
        self.path, self.records, self.sampled = path, records, sampled
        self.clusters: List[List[int]] = []       # file indices, the centre first
        self.status = "ok"

    def doc(self) -> Dict:
        n = len(self.sampled)
        return {"specimen": self.path, "reads": len(self.records), "sampled": n, "status": self.status,
                "clusters": [{"rank": r, "size": len(c), "share": round(len(c) / n, 4),
                              "centre": self.records[c[0]].id, "centre_length": len(self.records[c[0]].seq)}
                             for r, c in enumerate(self.clusters, 1)]}


def cluster_files(paths: Sequence[str], min_identity: float = 0.90, max_reads: int = 500, min_cluster_size: int = 5,
                  minor_share: float = 0.10, budget: Optional[int] = None,
                  adjacency_fn: Callable = adjacency, kernel_ms: Optional[list] = None) -> Tuple[List[SpecimenResult], Dict]:
    """Cluster every file of `paths` that can be read.  Returns the results in the order of `paths` and the summary
    {"specimens", "read", "failed", "mixed", "pairs"}."""
    sizes = []
    for p in paths:
        try:
            sizes.append(os.path.getsize(p))
        except OSError:
            sizes.append(0)
    results: List[Optional[SpecimenResult]] = [None] * len(paths)
    summary = {"specimens": len(paths), "read": 0, "failed": 0, "mixed": 0, "pairs": 0}
    for call in specimine.plan_calls([(s, []) for s in sizes], budget if budget is not None else budget_bytes()):
        batch: List[Tuple[int, SpecimenResult]] = []
        for i in call:
            try:
                records = read_records(paths[i])
            except (OSError, ValueError) as e:
                logging.error(f"Could not read {paths[i]}: {e}")
                summary["failed"] += 1
                continue
            batch.append((i, SpecimenResult(paths[i], records, sample_top_quality([r.qual for r in records], max_reads))))
        specimens = [([res.records[x].seq.encode("latin-1") for x in res.sampled],
                      [specimine.max_distance(len(res.records[x].seq), min_identity) for x in res.sampled])
                     for _, res in batch]
        adjs = adjacency_fn(specimens, kernel_ms) if specimens else []
        summary["pairs"] += pair_count(specimens)
        for (i, res), adj in zip(batch, adjs):
            quality = [mean_quality(res.records[x].qual) for x in res.sampled]
            res.clusters = [[res.sampled[x] for x in c] for c in star_clusters(adj, quality)]
            res.status = status_of([len(c) for c in res.clusters], len(res.sampled), min_cluster_size, minor_share)
            summary["read"] += 1
            summary["mixed"] += res.status == "mixed"
            results[i] = res
    return [r for r in results if r is not None], summary


def budget_bytes() -> int:
    env = os.environ.get("SMX_CLUSTERS_BUDGET_BYTES")
    return int(env) if env else specimine.budget_bytes()


# ------------------------------------------------------------------------------------------------ outputs
COLUMNS = ("specimen", "reads", "sampled", "status", "cluster", "size", "share", "centre", "centre_length")


def tsv_text(results: Sequence[SpecimenResult]) -> str:
    lines = ["\t".join(COLUMNS)]
    for res in results:
        d = res.doc()
        for c in d["clusters"]:
            lines.append("\t".join(str(x) for x in (d["specimen"], d["reads"], d["sampled"], d["status"], c["rank"],
                                                    c["size"], f"{c['share']:.4f}", c["centre"], c["centre_length"])))
    return "\n".join(lines) + "\n"


def json_text(results: Sequence[SpecimenResult], summary: Dict) -> str:
    return json.dumps({"summary": summary, "specimens": [r.doc() for r in results]}, indent=1) + "\n"


def below_full(path: str) -> str:
    """The path of a specimen file below its `full` directory (the first `full` component of the absolute path), the
    bare file name where there is none."""
    parts = os.path.abspath(path).split(os.sep)
    return os.sep.join(parts[parts.index("full") + 1:]) if "full" in parts[:-1] else parts[-1]


def centres_text(results: Sequence[SpecimenResult], min_cluster_size: int) -> str:
    out = []
    for res in results:
        name = specimine.extract_specimen_id(res.path)
        for rank, c in enumerate(res.clusters, 1):
            if len(c) >= min_cluster_size:
                rec = res.records[c[0]]
                out.append(f">{name}_c{rank} size={len(c)} share={len(c) / len(res.sampled):.4f} read={rec.id}\n{rec.seq}\n")
    return "".join(out)


def write_split(results: Sequence[SpecimenResult], min_cluster_size: int, out_dir: str) -> int:
    """DIR/<path below full/>/<S>.c<rank>.fastq per cluster of >= min_cluster_size reads: its records byte for byte as
    in the input, in input order.  Returns the number of files."""
    n = 0
    for res in results:
        rel = below_full(res.path)
        stem = rel[:-len(".fastq")] if rel.endswith(".fastq") else rel
        for rank, c in enumerate(res.clusters, 1):
            if len(c) < min_cluster_size:
                continue
            dest = os.path.join(out_dir, f"{stem}.c{rank}.fastq")
            os.makedirs(os.path.dirname(dest) or ".", exist_ok=True)
            with open(dest, "wb") as fh:
                for x in sorted(c):
                    raw = res.records[x].raw
                    fh.write(raw if raw.endswith(b"\n") else raw + b"\n")
            n += 1
    return n


def summary_line(summary: Dict) -> str:
    return (f"Clustered {summary['read']} of {summary['specimens']} specimen(s): {summary['mixed']} mixed; "
            f"{summary['pairs']} read pairs compared")


def run(args, adjacency_fn: Callable = adjacency, kernel_ms: Optional[list] = None) -> int:
    """Everything main() does after parsing; returns the exit status (1 only if no file could be read)."""
    paths = [args.fastq] if args.fastq else specimine.discover_specimens(args.run_dir, args.level)
    results, summary = cluster_files(paths, args.min_identity, args.max_reads, args.min_cluster_size, args.minor_share,
                                     adjacency_fn=adjacency_fn, kernel_ms=kernel_ms)
    if summary["read"] == 0:
        logging.error("No specimen file could be read")
        return 1
    for res in results:
        if res.status == "mixed":
            logging.info(f"mixed: {res.path}: clusters of {', '.join(str(len(c)) for c in res.clusters[:4])} reads"
                         f"{' ...' if len(res.clusters) > 4 else ''} of {len(res.sampled)} sampled")
    logging.info(summary_line(summary))
    if args.report:
        with open(args.report, "w", encoding="latin-1") as fh:
            fh.write(tsv_text(results))
    if args.json:
        with open(args.json, "w", encoding="latin-1") as fh:
            fh.write(json_text(results, summary))
    if args.centres:
        with open(args.centres, "w", encoding="latin-1") as fh:
            fh.write(centres_text(results, args.min_cluster_size))
    if args.split:
        write_split(results, args.min_cluster_size, args.split)
    return 0


def main(argv=None):
    specimine.tool_main(build_parser, run, argv)


if __name__ == "__main__":
    main()
