#!/usr/bin/env python3
"""specimux-errors: the error profile of a run's reads -- how often a base is substituted, inserted or deleted, how the
homopolymer runs come out, and whether the basecaller's Phred values mean what they say.  (The reference has no such tool.)

Every long-read tool here has a knob that stands in for one quantity, how noisy this run's reads are: --min-identity of
specimux-clusters / -consensus / -crosstalk, --min-separation, --min-site-share, the demultiplexer's own -e / -E.  This
tool measures it.  It runs specimux-consensus as it stands (consensus.consensus_files; with `--haplotypes`
specimux-variants, variants.variants_files), aligns the reads of every called sequence to the sequence once more, and
reduces the alignments, the sequence and the reads' quality strings on the device to counts (HIP kernels smx_cons.hip and
smx_profile.hip through smx_cons_profile, one call per planned device call; there is no CPU path).  All sums are integer
sums on the host; a float appears only where a number is formatted, each with a fixed format.

  column classes  match / sub (another base) / del (the read lacks the base) / other (a byte that is no base on either side)
  bases           the draft columns the aligned reads were compared at: match + sub + del + other
  rates           sub, ins (inserted bases), del and other per 1 000 bases
  identity        of a read: match / (match + sub + other + del + inserted bases); the report gives the 5th, 50th and 95th
                  percentile (nearest rank: the read of rank ceil(p n / 100) in ascending order)
  hp_off          the share of the draft's homopolymer runs of length >= 3, over all aligned reads, that a read shows at
                  another length
  not_aligned     the members of a called sequence that are above --min-identity in this tool's final alignment.  They
                  are counted and reported, never dropped silently
  clipped         reads with an insertion of 255 bases or more: counted everywhere but in the quality table, which needs
                  exact read positions

--min-identity: given, it serves the clustering, the polishing and the final alignment alike.  Not given, the clustering
and the polishing keep their own default (0.90) and the final alignment alone takes 0.80, so that the profile is not cut
off at the very limit it is meant to inform.

`implied` (--json) is a MODEL, not a measurement: what the measured rates would mean for the knobs if errors were
independent.  min_identity is the identity of the 5th-percentile read, floored to 0.01 -- the --min-identity that would
keep 95 % of this run's reads.  patterns gives, for each length of --pattern-lengths (primers, barcodes), the binomial
share of patterns of that length expected to carry more than e edits, e = 0..4, at the run's per-base error rate
(sub + other + del + inserted bases) / bases.

Limits.  The truth is the consensus of the same reads: an error the consensus shares is not seen.  Only the members of
the clusters are profiled, and those are drawn from the --max-reads best reads by mean quality: the run's worse reads are
not in the profile.

    python -m specimux_amd.errors --run-dir OUT --report E.tsv [--quality Q.tsv] [--homopolymers H.tsv] [--reads R.tsv]
        [--json J.json] [--haplotypes] [--pattern-lengths 13,20] [specimux-consensus' options; with --haplotypes
        specimux-variants']
    python -m specimux_amd.errors --fastq full/POOL/SPECIMEN.fastq [...]

One GPU."""
import functools
import json
import logging
import math
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import calls, clusters, consensus, specimine, variants

Job = consensus.Job
MEMBER_WORDS, Q_BINS, JOB_WORDS = 8, 64, 274              # smx.h: SMX_PROFILE_MEMBER_WORDS, _Q_BINS, _JOB_WORDS
Q, SUBST, INS, HP = 0, 192, 212, 218                      # the tables' offsets within a job's words
UPSTREAM_IDENTITY, FINAL_IDENTITY = 0.90, 0.80
DEFAULT_PATTERN_LENGTHS = "13,20"
MATCH, SUB, DEL, OTHER, INS_EVENTS, INS_BASES, CLIPPED = range(7)


def build_parser():
    parser = variants.build_parser()
    parser.description = "Measure the error profile of a run's reads against the consensus of their clusters."
    parser.add_argument("--haplotypes", action="store_true",
                        help="Run specimux-variants, with its options, instead of specimux-consensus: the reads of a split "
                             "cluster are compared with their own haplotype (names S_c1_h1)")
    parser.add_argument("--pattern-lengths", default=DEFAULT_PATTERN_LENGTHS,
                        help=f"Pattern lengths for the `implied` model of --json, comma separated (default: {DEFAULT_PATTERN_LENGTHS})")
    parser.add_argument("--quality", help="Write a TSV with one row per Phred value that has bases: bases, errors "
                                          "(sub + other + inserted), empirical and reported Q")
    parser.add_argument("--homopolymers", help="Write the run's table of true run length (1..7, 8+) against observed - true (-3..+3)")
    parser.add_argument("--reads", help="Write a TSV with one row per profiled read: its counts, identity and the error rate "
                                        "its own Phred string predicts")
    for action in parser._actions:
        if action.dest == "min_identity":
            action.default = None
            action.help = (f"Given: the limit of the clustering, the polishing and this tool's final alignment.  Not given: "
                           f"{UPSTREAM_IDENTITY:.2f} for the clustering and polishing, their own default, and {FINAL_IDENTITY:.2f} "
                           f"for the final alignment only, so that the profile is not cut off at the limit it is meant to inform")
        elif action.dest == "max_reads":
            action.help += ".  Only these reads' cluster members are profiled"
        elif action.dest == "report":
            action.help = "Write a TSV with one row per specimen and a `run` row"
        elif action.dest == "json":
            action.help = ("Write all of it as JSON, plus `implied`: a model, not a measurement, of what the rates mean for "
                           "--min-identity and for the edits a pattern of each --pattern-lengths is expected to carry.  The "
                           "truth is the consensus of the same reads, so errors the consensus shares are not seen")
        elif action.dest == "fasta":
            action.help = "Write the called sequences the reads were compared with"
        elif action.dest == "sites":
            action.help = "--haplotypes: write specimux-variants' TSV of kept sites"
    return parser


# ------------------------------------------------------------------------------------------------ the device call
class JobProfile(NamedTuple):
    """What one smx_cons_profile call returns for one job."""
    table: np.ndarray                      # (m + 1) x 26 votes, as consensus.votes returns them
    aligned: int
    members: np.ndarray                    # n x 8 uint32: match, sub, del, other, ins_events, ins_bases, clipped, 0
    tables: np.ndarray                     # 274 uint32: q[64][3], subst[4][5], ins[6], hp[8][7]


def profile(reads: Sequence[bytes], quals: Sequence[bytes], ks: Sequence[int], jobs: Sequence[Job],
            kernel_ms: Optional[list] = None) -> List[JobProfile]:
    """One smx_cons_profile call."""
    return [JobProfile(*job) for job in calls.cons_profile(reads, quals, ks, jobs, kernel_ms)]


# ------------------------------------------------------------------------------------------------ the numbers
def percentile_rank(p: int, n: int) -> int:
    """The index, in ascending order, of the p-th percentile of n values by nearest rank: ceil(p n / 100) - 1, at least 0."""
    return max((p * n + 99) // 100 - 1, 0)


def identity_parts(words: Sequence[int]) -> Tuple[int, int]:
    """(match, match + sub + other + del + inserted bases) of a read's eight counts."""
    return int(words[MATCH]), int(words[MATCH]) + int(words[SUB]) + int(words[OTHER]) + int(words[DEL]) + int(words[INS_BASES])


def identity_percentiles(parts: Sequence[Tuple[int, int]], ps: Sequence[int] = (5, 50, 95)) -> List[Optional[Tuple[int, int]]]:
    """The (match, denominator) of the reads at the percentiles `ps`; the order is that of the exact fractions (ties: the
    smaller denominator first).  None for each where there is no read."""
    if not parts:
        return [None] * len(ps)
    ordered = sorted(parts, key=functools.cmp_to_key(
        lambda a, b: (a[0] * b[1] > b[0] * a[1]) - (a[0] * b[1] < b[0] * a[1]) or (a[1] > b[1]) - (a[1] < b[1])))
    return [ordered[percentile_rank(p, len(ordered))] for p in ps]


def more_than(n: int, e: int, errors: int, bases: int) -> float:
    """The binomial share of patterns of n bases with more than e edits at the per-base rate errors / bases (at most 1)."""
    p = min(errors / bases, 1.0) if bases else 0.0
    return max(0.0, 1.0 - sum(math.comb(n, i) * p ** i * (1.0 - p) ** (n - i) for i in range(min(e, n) + 1)))


PHRED_ERROR = [10.0 ** (-max(b - 33, 0) / 10.0) for b in range(256)]       # the error probability a quality byte stands for


def predicted_error_permille(qual: str) -> Optional[float]:
    """The error rate a read's own Phred string predicts, per 1 000 bases: the mean of 10^(-Q / 10) over its bytes, summed
    as (bytes of each value) x (the value's probability) in the order of the values."""
    if not qual:
        return None
    counts = np.bincount(np.frombuffer(qual.encode("latin-1"), dtype=np.uint8), minlength=256).tolist()
    return 1000.0 * sum(n * PHRED_ERROR[b] for b, n in enumerate(counts) if n) / len(qual)


def fmt_identity(part: Optional[Tuple[int, int]]) -> str:
    return "-" if part is None or part[1] == 0 else f"{part[0] / part[1]:.4f}"


def fmt_rate(count: int, bases: int) -> str:
    return "-" if bases == 0 else f"{1000.0 * count / bases:.3f}"


class Totals:
    """Integer sums over reads and jobs: of one specimen, or of the run."""
    def __init__(self, name: str):
        self.name = name
        self.sequences = self.members = self.aligned = self.not_aligned = self.clipped = 0
        self.words = [0] * MEMBER_WORDS
        self.tables = np.zeros(JOB_WORDS, dtype=np.int64)
        self.parts: List[Tuple[int, int]] = []

    def add_job(self, jp: JobProfile) -> None:
        self.sequences += 1
        self.tables += jp.tables.astype(np.int64)
        for w in np.asarray(jp.members).tolist():
            self.members += 1
            if w[MATCH] + w[SUB] + w[DEL] + w[OTHER] == 0:   # a member above its limit: an aligned one has every draft column
                self.not_aligned += 1
                continue
            self.aligned += 1
            self.clipped += w[CLIPPED]
            for x in range(MEMBER_WORDS):
                self.words[x] += w[x]
            self.parts.append(identity_parts(w))

    @property
    def bases(self) -> int:
        return self.words[MATCH] + self.words[SUB] + self.words[DEL] + self.words[OTHER]

    @property
    def errors(self) -> int:
        return self.words[SUB] + self.words[OTHER] + self.words[DEL] + self.words[INS_BASES]

    def hp_long(self) -> Tuple[int, int]:
        """(runs of length >= 3 observed at another length, runs of length >= 3), over all aligned reads."""
        hp = self.tables[HP:].reshape(8, 7)[2:]
        return int(hp.sum() - hp[:, 3].sum()), int(hp.sum())


class Called:
    """One called sequence with the reads it was called from."""
    def __init__(self, result: int, specimen: str, name: str, seq: str, members: List[clusters.Read]):
        self.result, self.specimen, self.name, self.seq, self.members = result, specimen, name, seq, members
        self.profile: Optional[JobProfile] = None


def called_sequences(results, polished, phased) -> List[Called]:
    """support.called_sequences with the members as records: their quality strings are needed here."""
    out = []
    for i, res in enumerate(results):
        base = specimine.extract_specimen_id(res.path)
        for x, pc in enumerate(polished[i]):
            group = [res.records[r] for r in res.clusters[pc.rank - 1]]
            ph = phased[i][x] if phased is not None else None
            if ph is not None and ph.haps:
                for hap in ph.haps:
                    out.append(Called(i, res.path, f"{base}_c{pc.rank}_h{hap.index}", hap.seq, [group[m] for m in hap.members]))
            else:
                out.append(Called(i, res.path, f"{base}_c{pc.rank}", pc.seq, group))
    return out


def profile_cost(path_cost: int, called: Sequence[Called]) -> int:
    """consensus.specimen_cost extended by what the profile adds per called sequence: its members' quality bytes and
    counts, and its tables."""
    return path_cost + sum(4 * JOB_WORDS + sum(len(r.seq) + 4 * MEMBER_WORDS for r in c.members) for c in called)


# ------------------------------------------------------------------------------------------------ the run
def errors_files(paths: Sequence[str], args, final_identity: float, adjacency_fn: Callable = clusters.adjacency,
                 votes_fn: Callable = consensus.votes, phase_fn: Callable = variants.phase, profile_fn: Callable = profile,
                 kernel_ms: Optional[list] = None):
    """The upstream tool over `paths`, then per planned device call one profile_fn call over every called sequence (the
    draft) and its group's reads (the members), under the limit of `final_identity`.  Returns the upstream results, the
    called sequences with their profiles, variants' per-cluster records (None without --haplotypes) and the summary
    extended by {"profile_calls", "sequences"}."""
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
    summary = dict(summary, profile_calls=0, sequences=len(called))
    costs = [(profile_cost(consensus.specimen_cost(r.path, r, args.min_cluster_size), by_result[i]), [])
             for i, r in enumerate(results)]
    for call in specimine.plan_calls(costs, budget):
        todo = [c for i in sorted(call) for c in by_result[i]]
        if not todo:
            continue
        # the members of every sequence back to back, then every sequence: the draft of its job, whose quality is never read
        reads = [r.seq.encode("latin-1") for c in todo for r in c.members] + [c.seq.encode("latin-1") for c in todo]
        quals = [r.qual.encode("latin-1") for c in todo for r in c.members] + [b"!" * len(c.seq) for c in todo]
        ks = [specimine.max_distance(len(r), final_identity) for r in reads]
        jobs, at = [], 0
        for g, c in enumerate(todo):
            jobs.append((len(reads) - len(todo) + g, at, len(c.members)))
            at += len(c.members)
        summary["profile_calls"] += 1
        for c, jp in zip(todo, profile_fn(reads, quals, ks, jobs, kernel_ms)):
            c.profile = JobProfile(*jp)
    return results, called, phased, summary


def totals_of(results, called: Sequence[Called]) -> Tuple[List[Totals], Totals]:
    """Per specimen with a called sequence, in the order of the results, and the run."""
    run = Totals("run")
    per: Dict[int, Totals] = {}
    for c in called:
        t = per.setdefault(c.result, Totals(c.specimen))
        t.add_job(c.profile)
        run.add_job(c.profile)
    return [per[i] for i in sorted(per)], run


# ------------------------------------------------------------------------------------------------ outputs
COLUMNS = ("specimen", "sequences", "reads", "aligned", "not_aligned", "clipped", "bases", "sub_per_kb", "ins_per_kb",
           "del_per_kb", "other_per_kb", "identity_p5", "identity_p50", "identity_p95", "hp_off")
READ_COLUMNS = ("specimen", "name", "read", "match", "sub", "del", "other", "ins_events", "ins_bases", "clipped", "identity",
                "predicted_error_per_kb")
QUALITY_COLUMNS = ("q", "bases", "match", "sub_other", "inserted", "errors", "empirical_q", "reported_q")


def report_row(t: Totals) -> List[str]:
    off, long_runs = t.hp_long()
    b = t.bases
    return [t.name, str(t.sequences), str(t.members), str(t.aligned), str(t.not_aligned), str(t.clipped), str(b),
            fmt_rate(t.words[SUB], b), fmt_rate(t.words[INS_BASES], b), fmt_rate(t.words[DEL], b), fmt_rate(t.words[OTHER], b),
            *(fmt_identity(p) for p in identity_percentiles(t.parts)), "-" if long_runs == 0 else f"{off / long_runs:.4f}"]


def tsv_text(per: Sequence[Totals], run: Totals) -> str:
    return "\n".join(["\t".join(COLUMNS)] + ["\t".join(report_row(t)) for t in list(per) + [run]]) + "\n"


def empirical_q(errors: int, bases: int) -> str:
    return "inf" if errors == 0 else f"{-10.0 * math.log10(errors / bases):.2f}"


def quality_rows(run: Totals) -> List[List]:
    rows = []
    for b, (ok, bad, ins) in enumerate(run.tables[Q:Q + 3 * Q_BINS].reshape(Q_BINS, 3).tolist()):
        if ok + bad + ins:
            rows.append([b, ok + bad + ins, ok, bad, ins, bad + ins, empirical_q(bad + ins, ok + bad + ins), b])
    return rows


def quality_text(run: Totals) -> str:
    return "\n".join(["\t".join(QUALITY_COLUMNS)] + ["\t".join(str(x) for x in row) for row in quality_rows(run)]) + "\n"


def homopolymer_text(run: Totals) -> str:
    lines = ["\t".join(["true_length"] + [f"{d:+d}" if d else "0" for d in range(-3, 4)])]
    for r, row in enumerate(run.tables[HP:].reshape(8, 7).tolist()):
        lines.append("\t".join([str(r + 1) if r < 7 else "8+"] + [str(x) for x in row]))
    return "\n".join(lines) + "\n"


def read_rows(called: Sequence[Called]) -> List[List[str]]:
    rows = []
    for c in called:
        for rec, w in zip(c.members, np.asarray(c.profile.members).tolist()):
            aligned = w[MATCH] + w[SUB] + w[DEL] + w[OTHER] > 0
            predicted = predicted_error_permille(rec.qual)
            rows.append([c.specimen, c.name, rec.id, *(str(x) for x in w[:7]), fmt_identity(identity_parts(w)) if aligned else "-",
                         "-" if predicted is None else f"{predicted:.3f}"])
    return rows


def reads_text(rows: Sequence[Sequence[str]]) -> str:
    return "\n".join(["\t".join(READ_COLUMNS)] + ["\t".join(row) for row in rows]) + "\n"


def implied(run: Totals, lengths: Sequence[int]) -> Dict:
    p5 = identity_percentiles(run.parts, (5,))[0]
    return {"note": "a model, not a measurement: independent errors at the measured rates; the truth is the consensus of the same reads",
            "min_identity": None if p5 is None or p5[1] == 0 else f"{(100 * p5[0]) // p5[1] / 100:.2f}",
            "per_base_error_rate": None if run.bases == 0 else f"{min(run.errors / run.bases, 1.0):.6f}",
            "patterns": [{"length": n, "more_than": {str(e): f"{more_than(n, e, run.errors, run.bases):.6f}" for e in range(5)}}
                         for n in lengths]}


def totals_doc(t: Totals) -> Dict:
    doc = dict(zip(COLUMNS, report_row(t)))
    doc.update(counts=dict(zip(("match", "sub", "del", "other", "ins_events", "ins_bases"), t.words[:6])),
               subst=t.tables[SUBST:SUBST + 20].reshape(4, 5).tolist(), ins=t.tables[INS:INS + 6].tolist(),
               hp=t.tables[HP:].reshape(8, 7).tolist())
    return doc


def json_text(per: Sequence[Totals], run: Totals, rows: Sequence[Sequence[str]], summary: Dict, args, final_identity: float,
              lengths: Sequence[int]) -> str:
    settings = {"final_min_identity": final_identity, "min_identity": args.min_identity, "haplotypes": bool(args.haplotypes),
                "pattern_lengths": list(lengths), "max_reads": args.max_reads}
    return json.dumps({"summary": summary, "settings": settings, "run": totals_doc(run), "specimens": [totals_doc(t) for t in per],
                       "quality": [dict(zip(QUALITY_COLUMNS, row)) for row in quality_rows(run)],
                       "reads": [dict(zip(READ_COLUMNS, row)) for row in rows],
                       "implied": implied(run, lengths)}, indent=1) + "\n"


def fasta_text(called: Sequence[Called]) -> str:
    return "".join(f">{c.name} size={len(c.members)} aligned={c.profile.aligned}\n{c.seq}\n" for c in called)


def summary_line(summary: Dict, run: Totals) -> str:
    return (f"Profiled {run.aligned} read(s) of {summary['sequences']} sequence(s) of {summary['read']} specimen(s) in "
            f"{summary['profile_calls']} call(s): {run.not_aligned} not aligned, {run.clipped} clipped; per 1000 bases "
            f"{fmt_rate(run.words[SUB], run.bases)} sub, {fmt_rate(run.words[INS_BASES], run.bases)} ins, "
            f"{fmt_rate(run.words[DEL], run.bases)} del")


def parse_lengths(text: str) -> List[int]:
    lengths = sorted({int(x) for x in text.split(",") if x.strip()})
    if not lengths or any(n < 1 for n in lengths):
        raise ValueError("a pattern length must be at least 1")
    return lengths


def run(args, adjacency_fn: Callable = clusters.adjacency, votes_fn: Callable = consensus.votes,
        phase_fn: Callable = variants.phase, profile_fn: Callable = profile, kernel_ms: Optional[list] = None) -> int:
    """Everything main() does after parsing; returns the exit status (1 if no file could be read, 2 for a bad option)."""
    try:
        lengths = parse_lengths(args.pattern_lengths)
    except ValueError as exc:
        logging.error(f"--pattern-lengths: {exc}")
        return 2
    if args.min_identity is not None and not 0.0 <= args.min_identity <= 1.0:
        logging.error("--min-identity must be in 0..1")
        return 2
    if args.haplotypes and not 1 <= args.max_sites <= variants.MAX_SITES:
        logging.error(f"--max-sites must be in 1..{variants.MAX_SITES}")
        return 2
    final_identity = FINAL_IDENTITY if args.min_identity is None else args.min_identity
    if args.min_identity is None:
        args.min_identity = UPSTREAM_IDENTITY              # what the clustering and the polishing take when nothing is said
    paths = [args.fastq] if args.fastq else specimine.discover_specimens(args.run_dir, args.level)
    results, called, phased, summary = errors_files(paths, args, final_identity, adjacency_fn, votes_fn, phase_fn, profile_fn,
                                                    kernel_ms)
    if summary["read"] == 0:
        logging.error("No specimen file could be read")
        return 1
    per, total = totals_of(results, called)
    logging.info(summary_line(summary, total))
    rows = read_rows(called) if args.reads or args.json else []
    specimine.write_texts(((args.fasta, lambda: fasta_text(called)), (args.report, lambda: tsv_text(per, total)),
                           (args.quality, lambda: quality_text(total)), (args.homopolymers, lambda: homopolymer_text(total)),
                           (args.reads, lambda: reads_text(rows)),
                           (args.json, lambda: json_text(per, total, rows, summary, args, final_identity, lengths)),
                           (args.sites if phased is not None else None, lambda: variants.sites_text(results, phased))))
    return 0


def main(argv=None):
    specimine.tool_main(build_parser, run, argv)


if __name__ == "__main__":
    main()
