#!/usr/bin/env python3
"""specimux-support: how far each called sequence of a run can be trusted -- the resampling support of every base, and
the read depth at which the call would have been the same.  (The reference has no such tool.)

The tool runs specimux-consensus as it stands (consensus.consensus_files; with `--haplotypes` specimux-variants,
variants.variants_files) and then asks of every called sequence: draw many subsets of the reads it was called from,
vote again, and see whether each column, and the whole sequence, comes out as called.  The reads of a sequence are
aligned to it once; the votes of 64 subsets (replicates) at each of up to 16 depths (levels) are taken over the same
pileup rows, in one smx_cons_resample call per planned device call (HIP kernels smx_cons.hip and smx_resample.hip; there
is no CPU path).  A replicate keeps a column when consensus.call_consensus over its votes would emit there exactly what
the sequence has: no insertion before it, the base not dropped, the same base.

  level 0       the half sample: every replicate holds max(1, n // 2) of the sequence's n reads
  --depths      one more level per listed depth d: d reads per replicate.  Where n <= d the replicates are the whole group
                and the level is not applicable
  support       of a column: the replicates of level 0, out of 64, that keep it.  A replicate none of whose reads aligned
                keeps nothing
  weak          a column whose support is below --min-support (in 64ths, rounded up)
  whole         the replicates of a level that keep every column, and so reproduce the sequence
  stable_depth  the smallest listed depth d < n such that d and every larger applicable depth reproduce the sequence in at
                least --min-stable of the replicates
  status        unconverged (the full vote does not call the sequence itself: it is not a fixed point of the rule, and
                the support refers to a sequence the rule would change), else weak (some column is weak), else solid

The subsets do not depend on how specimens are packed into device calls: replicate b of a level is the d members with
the smallest (key, member index), the key a 64-bit integer mix of --seed, the CRC-32 of the sequence's name, the level's
tag (0 for the half sample, else d), b and the member index (subset_masks).  Sampling is without replacement, and the
support is relative to the final alignment: a replicate is not re-aligned to a draft of its own.

    python -m specimux_amd.support --run-dir OUT --report T.tsv [--json J.json] [--columns C.tsv] [--masked M.fasta]
        [--haplotypes] [--depths 3,5,10,20,50,100,200] [--min-support 0.95] [--min-stable 0.95] [--seed 1]
        [specimux-consensus' options; with --haplotypes specimux-variants']
    python -m specimux_amd.support --fastq full/POOL/SPECIMEN.fastq [...]

--masked writes the sequences with their weak columns in lower case, for viewing.  specimux-identify and specimux-bimera
compare bytes: give them the unmasked FASTA (--fasta).  One GPU."""
import json
import logging
import zlib
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import calls, clusters, consensus, specimine, variants

Job = consensus.Job
VOTE_WORDS = consensus.VOTE_WORDS
REPLICATES, MAX_LEVELS = 64, 16            # smx.h: SMX_CONS_REPLICATES, SMX_CONS_MAX_LEVELS
DEFAULT_DEPTHS = "3,5,10,20,50,100,200"
U64 = (1 << 64) - 1
GAMMA, MIX_A, MIX_B = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB   # splitmix64


def build_parser():
    parser = variants.build_parser()
    parser.description = "Resampling support of every base of each called sequence, and the depth its call needs."
    parser.add_argument("--haplotypes", action="store_true",
                        help="Run specimux-variants, with its options, instead of specimux-consensus: a split cluster's "
                             "sequences are its haplotypes, each resampled from its own reads (names S_c1_h1)")
    parser.add_argument("--depths", default=DEFAULT_DEPTHS,
                        help=f"Read depths to resample at, at most {MAX_LEVELS - 1}, comma separated.  The user's knob, not a "
                             f"measured constant (default: {DEFAULT_DEPTHS})")
    parser.add_argument("--min-support", type=float, default=0.95,
                        help="A column kept by a smaller share of the half-sample replicates is weak.  The user's knob, "
                             "not a measured constant (default: 0.95)")
    parser.add_argument("--min-stable", type=float, default=0.95,
                        help="Share of a depth's replicates that must reproduce the whole sequence for the depth to count "
                             "as enough.  The user's knob, not a measured constant (default: 0.95)")
    parser.add_argument("--seed", type=int, default=1, help="Seed of the subsets (default: 1)")
    parser.add_argument("--columns", help="Write a TSV with one row per weak column")
    for action in parser._actions:
        if action.dest == "fasta":
            action.help = "Write the called sequences, unmasked: the file for specimux-identify and specimux-bimera"
        elif action.dest == "report":
            action.help = "Write a TSV with one row per called sequence"
        elif action.dest == "json":
            action.help = "Write the same content as JSON, with the levels and the weak columns"
        elif action.dest == "sites":
            action.help = "--haplotypes: write specimux-variants' TSV of kept sites"
    parser.add_argument("--masked", help="Write the sequences with weak columns in lower case, for viewing only: "
                                         "specimux-identify and specimux-bimera compare bytes and should be given the "
                                         "unmasked FASTA (--fasta)")
    return parser


# ------------------------------------------------------------------------------------------------ the subsets
def _fin(z: int) -> int:
    """splitmix64's finaliser over a Python integer."""
    z &= U64
    z = ((z ^ (z >> 30)) * MIX_A) & U64
    z = ((z ^ (z >> 27)) * MIX_B) & U64
    return z ^ (z >> 31)


def _fin_array(z: np.ndarray) -> np.ndarray:
    """The same over a uint64 array; the products wrap."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX_A)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX_B)
    return z ^ (z >> np.uint64(31))


def subset_keys(seed: int, name: str, tag: int, n: int) -> np.ndarray:
    """key[b][i], 64 x n uint64, with fin = splitmix64's finaliser and all sums modulo 2^64:
        s = fin(seed + GAMMA);  t = fin(s + crc32(name) + GAMMA);  u = fin(t + tag + GAMMA)
        r[b] = fin(u + b + GAMMA);  key[b][i] = fin(r[b] + i + GAMMA)"""
    u = _fin(_fin(_fin(seed + GAMMA) + zlib.crc32(name.encode("latin-1")) + GAMMA) + tag + GAMMA)
    with np.errstate(over="ignore"):
        r = _fin_array(np.uint64(u) + np.arange(REPLICATES, dtype=np.uint64) + np.uint64(GAMMA))
        return _fin_array(r[:, None] + np.arange(n, dtype=np.uint64)[None, :] + np.uint64(GAMMA))


def subset_masks(seed: int, name: str, tag: int, n: int, d: int) -> np.ndarray:
    """One level's mask word per member: bit b is set when the member is among the d of replicate b, the d members with
    the smallest (key, member index).  d >= n: every member in every replicate."""
    if d >= n:
        return np.full(n, U64, dtype=np.uint64)
    order = np.argsort(subset_keys(seed, name, tag, n), axis=1, kind="stable")[:, :d]    # ties: the lower index
    chosen = np.zeros((REPLICATES, n), dtype=bool)
    chosen[np.arange(REPLICATES)[:, None], order] = True
    bits = np.left_shift(np.uint64(1), np.arange(REPLICATES, dtype=np.uint64))
    return np.bitwise_or.reduce(np.where(chosen, bits[:, None], np.uint64(0)), axis=0)


def level_depths(n: int, depths: Sequence[int]) -> List[Tuple[int, int, bool]]:
    """(tag, members per replicate, applicable) of every level of a group of n members: the half sample, then the depths."""
    return [(0, max(1, n // 2), True)] + [(d, min(d, n), d < n) for d in depths]


# ------------------------------------------------------------------------------------------------ the device call
class JobSupport(NamedTuple):
    """What one smx_cons_resample call returns for one job."""
    table: np.ndarray                      # (m + 1) x 26 votes, as consensus.votes returns them
    aligned: int
    agree: np.ndarray                      # n_levels x (m + 1) uint64: bit b = replicate b keeps the column
    sub_aligned: np.ndarray                # n_levels x 64 uint32: the replicates' voters


def resample(reads: Sequence[bytes], ks: Sequence[int], jobs: Sequence[Job], masks: np.ndarray,
             kernel_ms: Optional[list] = None) -> List[JobSupport]:
    """One smx_cons_resample call.  masks: n_levels x (the sum of the jobs' n) uint64, the jobs' members in job order
    (ValueError for another shape)."""
    return [JobSupport(*job) for job in calls.cons_resample(reads, ks, jobs, masks, kernel_ms)]


# ------------------------------------------------------------------------------------------------ the numbers
permille = specimine.permille


def need_of(share: float) -> int:
    """The replicates, out of 64, a share asks for: rounded up."""
    return (permille(share) * REPLICATES + 999) // 1000


def popcount(x: int) -> int:
    return bin(x).count("1")


class Column(NamedTuple):
    """One row of --columns."""
    pos: int
    kind: str                              # base | ins
    draft: str
    support: int
    alt: str
    alt_votes: int
    votes: int


class Called:
    """One called sequence and what the resampling says of it."""
    def __init__(self, result: int, specimen: str, name: str, seq: str, members: List[str]):
        self.result, self.specimen, self.name, self.seq, self.members = result, specimen, name, seq, members
        self.aligned = 0
        self.support: List[int] = []       # per column 0..m: the replicates of level 0 that keep it
        self.whole = 0
        self.levels: List[Dict] = []       # per listed depth {"depth", "applicable", "whole"}
        self.stable_depth: Optional[int] = None
        self.columns: List[Column] = []
        self.status = "solid"

    @property
    def half_depth(self) -> int:
        return max(1, len(self.members) // 2)


def level_numbers(agree_row: np.ndarray, sub_row: np.ndarray) -> Tuple[List[int], int]:
    """Per column the replicates that keep it, and the replicates that keep every column, of one level.  A replicate
    without voters counts as keeping nothing."""
    valid = sum(1 << b for b in range(REPLICATES) if int(sub_row[b]) > 0)
    words = [int(w) & valid for w in agree_row]
    whole = valid
    for w in words:
        whole &= w
    return [popcount(w) for w in words], popcount(whole)


def weak_rows(seq: str, p: int, support: int, row: Sequence[int], aligned: int) -> List[Column]:
    """The rows of a weak column p.  Which of the column's two tests can fail in a subset is read off the full vote: the
    insertion test only where some read has an insertion before p, the base test only where some read has something
    other than the draft's base at p.  Each gets a row with its runner-up in the full vote (ties: A C G T del)."""
    out = []
    m = len(seq)
    ins = sum(row[6:11])
    if p < m:
        dc = consensus.BASES.find(seq[p])
        options = [(row[c], -i, name) for i, (c, name) in enumerate(((0, "A"), (1, "C"), (2, "G"), (3, "T"), (5, "del")))
                   if c != dc]
        votes, _, alt = max(options)
        if votes > 0 or ins == 0:
            out.append(Column(p, "base", seq[p], support, alt if votes > 0 else "-", votes, aligned))
    if ins > 0 or not out:
        out.append(Column(p, "ins", "-", support, "ins", ins, aligned))
    return sorted(out, key=lambda c: c.kind != "base")


def evaluate(c: Called, js: JobSupport, depths: Sequence[int], need_support: int, need_stable: int) -> None:
    n = len(c.members)
    c.aligned = js.aligned
    c.support, c.whole = level_numbers(js.agree[0], js.sub_aligned[0])
    c.levels = []
    for l, (d, _, applicable) in enumerate(level_depths(n, depths)[1:], 1):
        c.levels.append({"depth": d, "applicable": applicable,
                         "whole": level_numbers(js.agree[l], js.sub_aligned[l])[1] if applicable else None})
    c.stable_depth = None
    for lv in sorted((lv for lv in c.levels if lv["applicable"]), key=lambda lv: -lv["depth"]):
        if lv["whole"] < need_stable:
            break
        c.stable_depth = lv["depth"]
    rows = np.asarray(js.table).tolist()
    c.columns = [col for p, s in enumerate(c.support) if s < need_support for col in weak_rows(c.seq, p, s, rows[p], js.aligned)]
    if consensus.call_consensus(c.seq, js.table, js.aligned) != c.seq:
        c.status = "unconverged"
    else:
        c.status = "weak" if any(s < need_support for s in c.support) else "solid"


# ------------------------------------------------------------------------------------------------ the run
def called_sequences(results, polished, phased) -> List[Called]:
    """Every called sequence with the reads it was called from: a polished cluster and its reads, or with `phased` the
    haplotypes of a split cluster, each with its own reads."""
    out = []
    for i, res in enumerate(results):
        base = specimine.extract_specimen_id(res.path)
        for x, pc in enumerate(polished[i]):
            group = [res.records[r].seq for r in res.clusters[pc.rank - 1]]
            ph = phased[i][x] if phased is not None else None
            if ph is not None and ph.haps:
                for hap in ph.haps:
                    out.append(Called(i, res.path, f"{base}_c{pc.rank}_h{hap.index}", hap.seq, [group[m] for m in hap.members]))
            else:
                out.append(Called(i, res.path, f"{base}_c{pc.rank}", pc.seq, group))
    return out


def support_cost(path_cost: int, called: Sequence[Called], n_levels: int) -> int:
    """consensus.specimen_cost extended by what the resampling adds per called sequence: the mask words of its members
    and its agree words."""
    return path_cost + sum(8 * n_levels * (len(c.members) + len(c.seq) + 1) for c in called)


def support_files(paths: Sequence[str], args, depths: Sequence[int], adjacency_fn: Callable = clusters.adjacency,
                  votes_fn: Callable = consensus.votes, phase_fn: Callable = variants.phase, resample_fn: Callable = resample,
                  kernel_ms: Optional[list] = None):
    """The upstream tool over `paths`, then per planned device call one resample_fn call over every called sequence (the
    draft) and its group's reads (the members).  Returns the upstream results, the called sequences, variants' per-cluster
    records (None without --haplotypes) and the summary extended by {"resample_calls", "sequences", "solid", "weak", "unconverged"}."""
    budget = clusters.budget_bytes()
    phased = None
    if args.haplotypes:
        results, polished, phased, summary = variants.variants_files(paths, args, adjacency_fn, votes_fn, phase_fn, kernel_ms)
    else:
        results, polished, summary = consensus.consensus_files(paths, args.min_identity, args.max_reads, args.min_cluster_size,
                                                               args.minor_share, args.rounds, budget=budget,
                                                               adjacency_fn=adjacency_fn, votes_fn=votes_fn, kernel_ms=kernel_ms)
    called = called_sequences(results, polished, phased)
    by_result: List[List[Called]] = [[] for _ in results]
    for c in called:
        by_result[c.result].append(c)
    n_levels = 1 + len(depths)
    need_support, need_stable = need_of(args.min_support), need_of(args.min_stable)
    summary = dict(summary, resample_calls=0, sequences=len(called), solid=0, weak=0, unconverged=0)
    costs = [(support_cost(consensus.specimen_cost(r.path, r, args.min_cluster_size), by_result[i], n_levels), [])
             for i, r in enumerate(results)]
    for call in specimine.plan_calls(costs, budget):
        todo = [c for i in sorted(call) for c in by_result[i]]
        if not todo:
            continue
        # the members of every sequence back to back, then every sequence: the draft of its job
        reads = [r.encode("latin-1") for c in todo for r in c.members] + [c.seq.encode("latin-1") for c in todo]
        ks = [specimine.max_distance(len(r), args.min_identity) for r in reads]
        jobs, at = [], 0
        for g, c in enumerate(todo):
            jobs.append((len(reads) - len(todo) + g, at, len(c.members)))
            at += len(c.members)
        masks = np.empty((n_levels, at), dtype=np.uint64)
        at = 0
        for c in todo:
            n = len(c.members)
            for l, (tag, d, _) in enumerate(level_depths(n, depths)):
                masks[l, at:at + n] = subset_masks(args.seed, c.name, tag, n, d)
            at += n
        summary["resample_calls"] += 1
        for c, js in zip(todo, resample_fn(reads, ks, jobs, masks, kernel_ms)):
            evaluate(c, js, depths, need_support, need_stable)
            summary[c.status] += 1
    return results, called, phased, summary


# ------------------------------------------------------------------------------------------------ outputs
COLUMNS = ("specimen", "name", "size", "aligned", "length", "half_depth", "min_support", "weak_columns", "whole",
           "stable_depth", "status")
WEAK_COLUMNS = ("name", "pos", "kind", "draft", "support", "alt", "alt_votes", "votes")


def weak_positions(c: Called, need_support: int) -> List[int]:
    return [p for p, s in enumerate(c.support) if s < need_support]


def doc(c: Called, need_support: int) -> Dict:
    return {"specimen": c.specimen, "name": c.name, "size": len(c.members), "aligned": c.aligned, "length": len(c.seq),
            "half_depth": c.half_depth, "min_support": min(c.support), "weak_columns": len(weak_positions(c, need_support)),
            "whole": c.whole, "stable_depth": c.stable_depth, "status": c.status,
            "levels": [{"depth": lv["depth"], "whole": lv["whole"]} for lv in c.levels],
            "columns": [col._asdict() for col in c.columns], "sequence": c.seq}


def tsv_text(called: Sequence[Called], need_support: int) -> str:
    lines = ["\t".join(COLUMNS)]
    for c in called:
        d = doc(c, need_support)
        lines.append("\t".join(str(x) for x in (
            d["specimen"], d["name"], d["size"], d["aligned"], d["length"], d["half_depth"], f"{d['min_support']}/{REPLICATES}",
            d["weak_columns"], f"{d['whole']}/{REPLICATES}", d["stable_depth"] if d["stable_depth"] is not None else "-",
            d["status"])))
    return "\n".join(lines) + "\n"


def columns_text(called: Sequence[Called]) -> str:
    lines = ["\t".join(WEAK_COLUMNS)]
    for c in called:
        for col in c.columns:
            lines.append("\t".join(str(x) for x in (c.name, col.pos, col.kind, col.draft, f"{col.support}/{REPLICATES}",
                                                    col.alt, col.alt_votes, col.votes)))
    return "\n".join(lines) + "\n"


def json_text(called: Sequence[Called], summary: Dict, args, depths: Sequence[int]) -> str:
    need_support = need_of(args.min_support)
    settings = {"depths": list(depths), "min_support": args.min_support, "min_stable": args.min_stable, "seed": args.seed,
                "need_support": need_support, "need_stable": need_of(args.min_stable), "replicates": REPLICATES,
                "haplotypes": bool(args.haplotypes)}
    return json.dumps({"summary": summary, "settings": settings, "sequences": [doc(c, need_support) for c in called]},
                      indent=1) + "\n"


def fasta_text(called: Sequence[Called]) -> str:
    return "".join(f">{c.name} size={len(c.members)} aligned={c.aligned} status={c.status}\n{c.seq}\n" for c in called)


def masked_text(called: Sequence[Called], need_support: int) -> str:
    """The sequences with their weak columns in lower case.  A weak column m, the insertion after the last base, has no
    base to show and appears in --columns only."""
    out = []
    for c in called:
        s = list(c.seq)
        for p in weak_positions(c, need_support):
            if p < len(s):
                s[p] = s[p].lower()
        out.append(f">{c.name} size={len(c.members)} aligned={c.aligned} status={c.status}\n{''.join(s)}\n")
    return "".join(out)


def summary_line(summary: Dict) -> str:
    return (f"Resampled {summary['sequences']} sequence(s) of {summary['read']} specimen(s) in {summary['resample_calls']} "
            f"call(s): {summary['solid']} solid, {summary['weak']} weak, {summary['unconverged']} unconverged")


def parse_depths(text: str) -> List[int]:
    depths = sorted({int(x) for x in text.split(",") if x.strip()})
    if any(d < 1 for d in depths):
        raise ValueError("a depth must be at least 1")
    return depths


def run(args, adjacency_fn: Callable = clusters.adjacency, votes_fn: Callable = consensus.votes,
        phase_fn: Callable = variants.phase, resample_fn: Callable = resample, kernel_ms: Optional[list] = None) -> int:
    """Everything main() does after parsing; returns the exit status (1 if no file could be read, 2 for a bad option)."""
    try:
        depths = parse_depths(args.depths)
    except ValueError as exc:
        logging.error(f"--depths: {exc}")
        return 2
    if len(depths) > MAX_LEVELS - 1:
        logging.error(f"--depths lists {len(depths)} depths; at most {MAX_LEVELS - 1} fit beside the half sample "
                      f"({MAX_LEVELS} levels per call)")
        return 2
    if args.haplotypes and not 1 <= args.max_sites <= variants.MAX_SITES:
        logging.error(f"--max-sites must be in 1..{variants.MAX_SITES}")
        return 2
    paths = [args.fastq] if args.fastq else specimine.discover_specimens(args.run_dir, args.level)
    results, called, phased, summary = support_files(paths, args, depths, adjacency_fn, votes_fn, phase_fn, resample_fn, kernel_ms)
    if summary["read"] == 0:
        logging.error("No specimen file could be read")
        return 1
    logging.info(summary_line(summary))
    need_support = need_of(args.min_support)
    specimine.write_texts(((args.fasta, lambda: fasta_text(called)), (args.report, lambda: tsv_text(called, need_support)),
                           (args.json, lambda: json_text(called, summary, args, depths)), (args.columns, lambda: columns_text(called)),
                           (args.masked, lambda: masked_text(called, need_support)),
                           (args.sites if phased is not None else None, lambda: variants.sites_text(results, phased))))
    return 0


def main(argv=None):
    specimine.tool_main(build_parser, run, argv)


if __name__ == "__main__":
    main()
