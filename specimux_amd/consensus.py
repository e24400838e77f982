#!/usr/bin/env python3
"""specimux-consensus: one polished consensus sequence per cluster of a demultiplexed specimen.  (The reference has no
such tool: it hands this step to an external consensus program.)

The clusters are specimux-clusters' (clusters.cluster_files, unchanged): per specimen file the sampled reads, star
clusters around centre reads.  Every cluster of at least `--min-cluster-size` reads is polished in rounds.  The draft of
the first round is the centre read.  In a round every read of the cluster, the centre included, is aligned globally to
the draft -- NW with traceback, limited to max(k[draft], k[read]) with k = int(len * (1 - min_identity)) -- and the
alignments are reduced to per-position votes; both happen on the GPU (smx_cons_votes, HIP kernels smx_cons.hip), for all
clusters of all specimens of a device call at once; there is no CPU path.  The host then calls the next draft from the
votes (call_consensus, integers only).  The rounds of a cluster stop when the draft no longer changes (`converged`),
after `--rounds` (`rounds`), when fewer than `--min-cluster-size` reads aligned within their limit (`low_aligned`: the
last draft is kept) or when the call would be empty (`empty`: the previous draft is kept).

    python -m specimux_amd.consensus --fastq full/POOL/SPECIMEN.fastq --fasta OUT.fasta [--report R.tsv] [--json R.json]
        [--rounds 3] [--min-identity 0.90] [--max-reads 500] [--min-cluster-size 5] [--minor-share 0.10]
    python -m specimux_amd.consensus --run-dir OUT [--level pool|primer-pair] [...]

Device calls are planned under clusters' byte budget (SMX_CLUSTERS_BUDGET_BYTES, else specimine's); a specimen costs
its file plus the pileup rows of its polished clusters, which stay on the device.  The alignment history of the
workgroups in flight is a workspace of the library's own, bounded there.  One GPU."""
import argparse
import json
import logging
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import calls, clusters, specimine

MAX_INS, VOTE_WORDS = 4, 26                # smx.h: SMX_CONS_MAX_INS, SMX_CONS_VOTE_WORDS
BASES = "ACGT"
Job = Tuple[int, int, int]                 # (draft, r0, n): indices into the call's read list


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Polish one consensus sequence per cluster of each specimen.")
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("--fastq", help="Path to one specimen's FASTQ file")
    source.add_argument("--run-dir", help="specimux output directory: every specimen file under RUN_DIR/full/")
    parser.add_argument("--level", choices=("pool", "primer-pair"), default="pool",
                        help="--run-dir: full/<pool>/<S>.fastq (pool) or full/<pool>/<pair>/<S>.fastq (default: pool)")
    parser.add_argument("--min-identity", type=float, default=0.90,
                        help="As in specimux-clusters; also the limit of a read's alignment to the draft (default: 0.90)")
    parser.add_argument("--max-reads", type=int, default=500,
                        help="Use at most this many reads per specimen, the best by mean quality (default: 500)")
    parser.add_argument("--min-cluster-size", type=int, default=5,
                        help="Smallest cluster that is polished, and smallest number of aligned reads a round may call "
                             "from (default: 5)")
    parser.add_argument("--minor-share", type=float, default=0.10,
                        help="As in specimux-clusters: the share of the second cluster that makes a specimen mixed "
                             "(default: 0.10)")
    parser.add_argument("--rounds", type=int, default=3, help="Polishing rounds per cluster at most (default: 3)")
    parser.add_argument("--fasta", help="Write one record per polished cluster")
    parser.add_argument("--report", help="Write a TSV with one row per polished cluster")
    parser.add_argument("--json", help="Write the same content as JSON, with the sequences")
    parser.add_argument("--debug", action="store_true", help="Enable debug logging")
    return parser


# ------------------------------------------------------------------------------------------------ votes
votes = calls.cons_votes


# ------------------------------------------------------------------------------------------------ the call rule
def call_consensus(draft: str, table: np.ndarray, aligned: int) -> str:
    """The next draft from the votes of `aligned` reads over `draft` (table[p] = sym[6], then ins[slot][code]).  Integer
    arithmetic only.  Before position p (and after the last base, p = len(draft)) the insertion slots 0, 1, ... are
    emitted while more than half of the reads vote in the slot, each as the ACGT code with the most votes there (ties:
    the lowest code).  At position p the base is dropped if more than half of the reads have a deletion; otherwise it is
    the ACGT code with the most votes -- on a tie the draft's own base if it is among the tied, else the lowest code --
    and the draft's own base where no read votes ACGT at all."""
    n = int(aligned)
    out = []
    rows = np.asarray(table).tolist()
    for p in range(len(draft) + 1):
        v = rows[p]
        for s in range(MAX_INS):
            slot = v[6 + 5 * s:11 + 5 * s]
            if 2 * sum(slot) <= n:
                break
            out.append(BASES[max(range(4), key=lambda c: (slot[c], -c))])
        if p == len(draft) or 2 * v[5] > n:
            continue
        top = max(v[:4])
        if top == 0:
            out.append(draft[p])
            continue
        tied = [c for c in range(4) if v[c] == top]
        out.append(draft[p] if draft[p] in [BASES[c] for c in tied] else BASES[tied[0]])
    return "".join(out)


def nw_distance(a: str, b: str) -> int:
    """Global edit distance of two strings, row by row over numpy: the within-row dependency D[j] = min(x[j], D[j-1] + 1)
    is a running minimum of x[j] - j."""
    ta = np.frombuffer(a.encode("latin-1"), dtype=np.uint8)
    tb = np.frombuffer(b.encode("latin-1"), dtype=np.uint8)
    idx = np.arange(len(tb) + 1, dtype=np.int64)
    row = idx.copy()
    for i, c in enumerate(ta, 1):
        x = np.empty_like(row)
        x[0] = i
        np.minimum(row[:-1] + (tb != c), row[1:] + 1, out=x[1:])
        row = np.minimum.accumulate(x - idx) + idx
    return int(row[-1])


# ------------------------------------------------------------------------------------------------ polishing
class Polished:
    """One polished cluster of a specimen."""
    def __init__(self, rank: int, size: int, centre: str):
        self.rank, self.size, self.centre = rank, size, centre
        self.seq = centre
        self.aligned = 0        # the reads that voted in the last round
        self.rounds = 0         # vote rounds run
        self.stop = "rounds"    # converged | rounds | low_aligned | empty
        self.edits = 0          # NW distance centre -> consensus


def polish(groups: Sequence[Sequence[str]], min_identity: float, rounds: int, min_aligned: int,
           votes_fn: Callable = votes, kernel_ms: Optional[list] = None,
           drafts: Optional[Sequence[str]] = None) -> Tuple[List[Tuple[str, int, int, str]], int]:
    """Polish every group (a cluster's reads, the centre first) of one device call.  A round is one votes_fn call over
    the groups still running: the read list holds the groups back to back, then the drafts later rounds added.  Draft 0
    of a group is its first member, or drafts[g] where `drafts` is given: such a draft is not a member and does not
    vote.  Returns per group (consensus, aligned, rounds, stop), and the number of votes_fn calls."""
    reads = [r.encode("latin-1") for g in groups for r in g]
    first, at = [], 0
    for g in groups:
        first.append(at)
        at += len(g)
    if drafts is None:
        drafts = [g[0] for g in groups]
        draft_at = list(first)                                 # the centre is the first member
    else:
        drafts = list(drafts)
        draft_at = [len(reads) + g for g in range(len(groups))]
        reads += [d.encode("latin-1") for d in drafts]
    ks = [specimine.max_distance(len(r), min_identity) for r in reads]
    state = [[0, 0, "rounds"] for _ in groups]                 # aligned, rounds, stop
    live = list(range(len(groups)))
    n_calls = 0
    for _ in range(max(rounds, 0)):
        if not live:
            break
        n_calls += 1
        jobs = [(draft_at[g], first[g], len(groups[g])) for g in live]
        tables, aligned = votes_fn(reads, ks, jobs, kernel_ms)
        still = []
        for g, table, n in zip(live, tables, aligned):
            state[g][0], state[g][1] = n, state[g][1] + 1
            if n < min_aligned:
                state[g][2] = "low_aligned"
                continue
            new = call_consensus(drafts[g], table, n)
            if not new:
                state[g][2] = "empty"
            elif new == drafts[g]:
                state[g][2] = "converged"
            else:
                drafts[g] = new
                draft_at[g] = len(reads)
                reads.append(new.encode("latin-1"))
                ks.append(specimine.max_distance(len(new), min_identity))
                still.append(g)
        live = still
    return [(drafts[g], state[g][0], state[g][1], state[g][2]) for g in range(len(groups))], n_calls


def specimen_cost(path: str, res: clusters.SpecimenResult, min_cluster_size: int) -> int:
    """What a specimen adds to a device call: its file and the pileup rows of its polished clusters."""
    try:
        size = os.path.getsize(path)
    except OSError:
        size = 0
    return size + sum(4 * len(c) * (len(res.records[c[0]].seq) + 1) for c in res.clusters if len(c) >= min_cluster_size)


def consensus_files(paths: Sequence[str], min_identity: float = 0.90, max_reads: int = 500, min_cluster_size: int = 5,
                    minor_share: float = 0.10, rounds: int = 3, budget: Optional[int] = None,
                    adjacency_fn: Callable = clusters.adjacency, votes_fn: Callable = votes,
                    kernel_ms: Optional[list] = None) -> Tuple[List[clusters.SpecimenResult], List[List[Polished]], Dict]:
    """Cluster every file of `paths` (clusters.cluster_files) and polish every cluster of >= min_cluster_size reads.
    Returns clusters' results, per result its polished clusters, and clusters' summary extended by {"polished",
    "vote_calls"}."""
    budget = budget if budget is not None else clusters.budget_bytes()
    results, summary = clusters.cluster_files(paths, min_identity, max_reads, min_cluster_size, minor_share, budget=budget,
                                              adjacency_fn=adjacency_fn)
    polished: List[List[Polished]] = [[] for _ in results]
    summary = dict(summary, polished=0, vote_calls=0)
    for call in specimine.plan_calls([(specimen_cost(r.path, r, min_cluster_size), []) for r in results], budget):
        groups, owner = [], []
        for i in sorted(call):
            res = results[i]
            for rank, c in enumerate(res.clusters, 1):
                if len(c) >= min_cluster_size:
                    groups.append([res.records[x].seq for x in c])
                    owner.append((i, rank))
        if not groups:
            continue
        done, n_calls = polish(groups, min_identity, rounds, min_cluster_size, votes_fn, kernel_ms)
        summary["vote_calls"] += n_calls
        for (i, rank), g, (seq, aligned, nrounds, stop) in zip(owner, groups, done):
            pc = Polished(rank, len(g), g[0])
            pc.seq, pc.aligned, pc.rounds, pc.stop = seq, aligned, nrounds, stop
            pc.edits = nw_distance(g[0], seq) if seq != g[0] else 0
            polished[i].append(pc)
            summary["polished"] += 1
    return results, polished, summary


# ------------------------------------------------------------------------------------------------ outputs
COLUMNS = ("specimen", "status", "sampled", "cluster", "size", "share", "aligned", "rounds", "stop", "edits", "length", "name")


def cluster_docs(res: clusters.SpecimenResult, pcs: Sequence[Polished]) -> List[Dict]:
    name = specimine.extract_specimen_id(res.path)
    return [{"name": f"{name}_c{pc.rank}", "rank": pc.rank, "size": pc.size, "share": round(pc.size / len(res.sampled), 4),
             "aligned": pc.aligned, "rounds": pc.rounds, "stop": pc.stop, "edits": pc.edits, "length": len(pc.seq),
             "consensus": pc.seq} for pc in pcs]


def fasta_text(results: Sequence[clusters.SpecimenResult], polished: Sequence[Sequence[Polished]]) -> str:
    out = []
    for res, pcs in zip(results, polished):
        for d in cluster_docs(res, pcs):
            out.append(f">{d['name']} size={d['size']} share={d['share']:.4f} aligned={d['aligned']} rounds={d['rounds']} "
                       f"edits={d['edits']}\n{d['consensus']}\n")
    return "".join(out)


def tsv_text(results: Sequence[clusters.SpecimenResult], polished: Sequence[Sequence[Polished]]) -> str:
    lines = ["\t".join(COLUMNS)]
    for res, pcs in zip(results, polished):
        for d in cluster_docs(res, pcs):
            lines.append("\t".join(str(x) for x in (res.path, res.status, len(res.sampled), d["rank"], d["size"],
                                                    f"{d['share']:.4f}", d["aligned"], d["rounds"], d["stop"], d["edits"],
                                                    d["length"], d["name"])))
    return "\n".join(lines) + "\n"


def json_text(results: Sequence[clusters.SpecimenResult], polished: Sequence[Sequence[Polished]], summary: Dict) -> str:
    return json.dumps({"summary": summary,
                       "specimens": [{"specimen": res.path, "reads": len(res.records), "sampled": len(res.sampled),
                                      "status": res.status, "clusters": cluster_docs(res, pcs)}
                                     for res, pcs in zip(results, polished)]}, indent=1) + "\n"


def summary_line(summary: Dict) -> str:
    return (f"Polished {summary['polished']} cluster(s) of {summary['read']} specimen(s) ({summary['mixed']} mixed) in "
            f"{summary['vote_calls']} vote call(s)")


def run(args, adjacency_fn: Callable = clusters.adjacency, votes_fn: Callable = votes, kernel_ms: Optional[list] = None) -> int:
    """Everything main() does after parsing; returns the exit status (1 only if no file could be read)."""
    paths = [args.fastq] if args.fastq else specimine.discover_specimens(args.run_dir, args.level)
    results, polished, summary = consensus_files(paths, args.min_identity, args.max_reads, args.min_cluster_size,
                                                 args.minor_share, args.rounds, adjacency_fn=adjacency_fn,
                                                 votes_fn=votes_fn, kernel_ms=kernel_ms)
    if summary["read"] == 0:
        logging.error("No specimen file could be read")
        return 1
    for res, pcs in zip(results, polished):
        for pc in pcs:
            if pc.stop == "low_aligned":
                logging.warning(f"{res.path}: cluster {pc.rank}: only {pc.aligned} of {pc.size} reads aligned to the draft of "
                                f"round {pc.rounds}; the draft is kept as it was")
    logging.info(summary_line(summary))
    specimine.write_texts(((args.fasta, lambda: fasta_text(results, polished)), (args.report, lambda: tsv_text(results, polished)),
                           (args.json, lambda: json_text(results, polished, summary))))
    return 0


def main(argv=None):
    specimine.tool_main(build_parser, run, argv)


if __name__ == "__main__":
    main()
