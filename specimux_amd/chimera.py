"""specimux-chimera: find primers INSIDE reads and flag concatemers (not in the reference: it looks for primers and
barcodes only in the first and last `search_len` bases of a read, so two amplicons ligated into one read

    [bc_f1][P_fwd] ...A... [rc P_rev][rc bc_r1][bc_f2][P_fwd] ...B... [rc P_rev][rc bc_r2]

demultiplex as (f1, r2): a full match for the wrong specimen, or a partial one that specimine may pull into a bin).

Every primer of the panel, as written (strand +) and reverse-complemented (strand -), is aligned against the whole
read on the GPU (libsmx smx_inner_scan); a hit is a place outside the two end windows where it
matches within its threshold.  In either read orientation an amplicon opens with a primer as written and closes with a
reverse-complemented one, so a junction is a `-` hit followed closely by a `+` hit: that is the default flag rule.

    python -m specimux_amd.chimera primers.fasta specimens.txt reads.fastq[.gz]
           [-E N] [-l N] [-n N] [--inner-edit-distance 3] [--junction-gap 100] [--flag-rule junction|any]
           [--report FILE.tsv] [--clean FILE] [--flagged FILE]

The file streams through the native reader in batches; nothing here grows with the file.  The clean / flagged files
are written by libsmx from the batch, whole header lines included."""
import argparse
import logging
import sys
import timeit
from typing import NamedTuple

import numpy as np

from . import calls

BATCH_READS = 65536         # reads per scan call on the file path
BATCH_BYTES = 64 << 20      # and at most about this many bases
REPORT_HEADER = "read_id\tlength\tprimer\tstrand\tdistance\tend\tread_flagged\n"
RULES = ("junction", "any")


class PatternInfo(NamedTuple):
    name: str      # primer name
    strand: str    # "+" as written, "-" reverse complement
    seq: str       # the searched pattern
    k: int         # its threshold


def panel_patterns(specimens, parameters, inner_k):
    """The scan's patterns for a loaded panel: for primer i in Specimens._primers order, pattern 2i is the primer as written
    and 2i + 1 its reverse complement; k = min(the primer's demux threshold, inner_k), below the primer's length."""
    out = []
    for info in specimens._primers.values():
        k = min(int(parameters.max_dist_primers[info.primer]), int(inner_k), len(info.primer) - 1)
        out.append(PatternInfo(info.name, "+", info.primer, max(k, 0)))
        out.append(PatternInfo(info.name, "-", info.primer_rc, max(k, 0)))
    return out


def _seqs(patterns):
    return [p.seq if isinstance(p, PatternInfo) else p for p in patterns]


def scan(bases, offsets, patterns, k, margin, max_hits=4, budget_bytes=0, kernel_ms=None):
    """calls.inner_scan; a pattern may be a PatternInfo or its sequence."""
    return calls.inner_scan(bases, offsets, _seqs(patterns), k, margin, max_hits, budget_bytes, kernel_ms)


def scan_batch(batch, patterns, k, margin, max_hits=4, budget_bytes=0, kernel_ms=None):
    """calls.inner_scan_batch; a pattern may be a PatternInfo or its sequence."""
    return calls.inner_scan_batch(batch, _seqs(patterns), k, margin, max_hits, budget_bytes, kernel_ms)


def flag_reads(nhit, hit_dist, hit_end, pattern_info, rule="junction", gap=100):
    """Per read: flagged or not (numpy bool).  Rule `any`: at least one hit.  Rule `junction`: a `-` hit a and a `+` hit b
    with -k_b <= (end_b - len(pattern_b) + 1) - (end_a + 1) <= gap, i.e. a closing primer followed, at most `gap` bases on
    (or overlapping by no more than b's threshold, which is how far its nominal start can be off), by an opening one.
    Only the stored hits (the first H per read and pattern) take part."""
    if rule not in RULES:
        raise ValueError(f"unknown flag rule {rule!r}")
    nhit = np.asarray(nhit)
    hit_end = np.asarray(hit_end)
    any_hit = nhit.any(axis=1) if nhit.size else np.zeros(len(nhit), dtype=bool)
    if rule == "any":
        return any_hit
    H = hit_end.shape[2] if hit_end.ndim == 3 else 0
    minus = [j for j, p in enumerate(pattern_info) if p.strand == "-"]
    plus = [j for j, p in enumerate(pattern_info) if p.strand == "+"]
    flagged = np.zeros(len(nhit), dtype=bool)
    if not minus or not plus:
        return flagged
    # candidates: reads with a hit of each strand (few); the pair test runs on those alone
    cand = np.flatnonzero(nhit[:, minus].any(axis=1) & nhit[:, plus].any(axis=1))
    for r in cand:
        closes = [int(hit_end[r, j, h]) + 1 for j in minus for h in range(min(int(nhit[r, j]), H))]
        for j in plus:
            p = pattern_info[j]
            for h in range(min(int(nhit[r, j]), H)):
                start = int(hit_end[r, j, h]) - len(p.seq) + 1
                if any(-p.k <= start - c <= gap for c in closes):
                    flagged[r] = True
                    break
            if flagged[r]:
                break
    return flagged


def report_rows(read_ids, lengths, nhit, hit_dist, hit_end, pattern_info, flagged, reads=None):
    """Report lines (no header) for the reads `reads` (indices, default: every read with a hit), in that order, then by
    pattern, then by hit (column order).  read_ids / lengths: mappings or sequences indexed by read."""
    H = hit_end.shape[2]
    if reads is None:
        reads = np.flatnonzero(np.asarray(nhit).any(axis=1))
    rows = []
    for r in reads:
        r = int(r)
        for j, p in enumerate(pattern_info):
            for h in range(min(int(nhit[r, j]), H)):
                rows.append(f"{read_ids[r]}\t{lengths[r]}\t{p.name}\t{p.strand}\t{int(hit_dist[r, j, h])}\t"
                            f"{int(hit_end[r, j, h])}\t{1 if flagged[r] else 0}\n")
    return rows


def build_parser():
    ap = argparse.ArgumentParser(
        prog="specimux-chimera",
        description="Find primers inside reads (outside the end windows specimux searches) and flag concatemers.")
    ap.add_argument("primer_file", help="Fasta file containing primer information")
    ap.add_argument("specimen_file", help="TSV file containing specimen mapping with barcodes and primers")
    ap.add_argument("sequence_file", help="Sequence file in Fasta or Fastq format, gzipped or plain text")
    ap.add_argument("-n", "--num-seqs", type=str, default="-1", help="Number of sequences to read from file (e.g., -n 100 or -n 102,3)")
    ap.add_argument("-e", "--index-edit-distance", type=int, default=-1, help="Barcode edit distance value, as for specimux")
    ap.add_argument("-E", "--primer-edit-distance", type=int, default=-1, help="Primer edit distance value, as for specimux")
    ap.add_argument("-l", "--search-len", type=int, default=80,
                    help="The end windows specimux searches (default: 80): only hits outside them are reported")
    ap.add_argument("--inner-edit-distance", type=int, default=3, metavar="N",
                    help="Largest edit distance of a primer hit inside a read (default 3; never above the primer's own threshold)")
    ap.add_argument("--junction-gap", type=int, default=100, metavar="N",
                    help="Rule junction: at most this many bases between a closing and the next opening primer (default 100)")
    ap.add_argument("--flag-rule", choices=RULES, default="junction",
                    help="junction: a reverse-complemented primer followed closely by a primer as written (default); any: any hit")
    ap.add_argument("--max-hits", type=int, default=4, metavar="H", help="Hits kept per read and primer orientation (1-8, default 4)")
    ap.add_argument("--report", metavar="FILE.tsv", help="Write one row per hit")
    ap.add_argument("--clean", metavar="FILE", help="Write the records that were not flagged (untrimmed), to feed to specimux")
    ap.add_argument("--flagged", metavar="FILE", help="Write the flagged records (untrimmed)")
    ap.add_argument("-D", "--debug", action="store_true", help="Enable debug logging")
    return ap


def parse_args(argv):
    from .cli import split_num_seqs
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.inner_edit_distance < 0:
        ap.error("--inner-edit-distance must not be negative")
    if args.junction_gap < 0:
        ap.error("--junction-gap must not be negative")
    if args.search_len < 0:
        ap.error("--search-len must not be negative")
    if not 1 <= args.max_hits <= 8:
        ap.error("--max-hits must be between 1 and 8")
    return split_num_seqs(ap, args)


def load_panel(args):
    """Panel and thresholds as specimux_amd.cli reads them."""
    from .io_utils import read_primers_file, read_specimen_file
    from .orchestration import setup_match_parameters
    registry = read_primers_file(args.primer_file)
    specimens = read_specimen_file(args.specimen_file, registry)
    specimens.validate()
    ns = argparse.Namespace(index_edit_distance=args.index_edit_distance, primer_edit_distance=args.primer_edit_distance,
                            search_len=args.search_len, dereplicate="best", disable_preorient=False,
                            disable_prefilter=True, diagnostics=None)
    return specimens, setup_match_parameters(ns, specimens)


def run(args, timings=None):
    """The whole tool for parsed arguments.  Returns (reads scanned, reads with hits, reads flagged, hits per pattern)."""
    from .native_io import Reader
    specimens, parameters = load_panel(args)
    info = panel_patterns(specimens, parameters, args.inner_edit_distance)
    ks = [p.k for p in info]
    for p in info[::2]:
        logging.info(f"Inner scan threshold {p.k} for primer {p.name} ({p.seq})")
    reader = Reader(args.sequence_file)
    # ids are bytes of the input decoded as latin-1: written back the same way, whatever the locale
    report = open(args.report, "w", encoding="latin-1", newline="") if args.report else None
    for path in (args.clean, args.flagged):   # the native writer appends batch by batch
        if path:
            open(path, "wb").close()
    if report:
        report.write(REPORT_HEADER)
    total = with_hits = n_flagged = 0
    per_pattern = np.zeros(len(info), dtype=np.int64)
    kernel_ms, split_s = [], 0.0
    to_skip = max(0, args.start_seq - 1)
    left = args.num_seqs if args.num_seqs >= 0 else None
    batch = None
    try:
        while left is None or left > 0:
            want = BATCH_READS if left is None else min(BATCH_READS, left)
            if to_skip > 0:   # -n start,num: discard the first start - 1 records
                batch = reader.next_batch(min(to_skip, BATCH_READS), BATCH_BYTES, into=batch)
                if batch is None:
                    break
                to_skip -= len(batch)
                continue
            batch = reader.next_batch(want, BATCH_BYTES, into=batch)
            if batch is None:
                break
            n = len(batch)
            nhit, dist, end = scan_batch(batch, info, ks, args.search_len, args.max_hits, kernel_ms=kernel_ms)
            flags = flag_reads(nhit, dist, end, info, args.flag_rule, args.junction_gap)
            hit_reads = np.flatnonzero(nhit.any(axis=1))
            total += n
            with_hits += len(hit_reads)
            n_flagged += int(flags.sum())
            per_pattern += nhit.sum(axis=0, dtype=np.int64)
            if left is not None:
                left -= n
            if report and len(hit_reads):
                ids, lens = {}, {}
                for r in hit_reads:
                    rid, seq, _ = batch.record(int(r))
                    ids[int(r)], lens[int(r)] = rid, len(seq)
                report.writelines(report_rows(ids, lens, nhit, dist, end, info, flags, hit_reads))
            if args.clean or args.flagged:
                t0 = timeit.default_timer()
                batch.write_split(flags, args.clean, args.flagged)
                split_s += timeit.default_timer() - t0
    finally:
        if report:
            report.close()
        if batch is not None:
            batch.close()
        reader.close()
    if timings is not None:
        timings.update(kernel_ms=float(sum(kernel_ms)), split_s=split_s)
    return total, with_hits, n_flagged, [(p, int(c)) for p, c in zip(info, per_pattern)]


def main(argv=None):
    """Entry point; argv without the program name.  Returns the exit status (0 also when nothing is flagged)."""
    from .cli import setup_logging, version
    args = parse_args(sys.argv[1:] if argv is None else argv)
    setup_logging(args.debug)
    logging.info(f"Starting specimux-chimera, {version()}")
    start = timeit.default_timer()
    timings = {}
    total, with_hits, n_flagged, per_pattern = run(args, timings)
    counts = ", ".join(f"{p.name}{p.strand} {c}" for p, c in per_pattern)
    logging.info(f"Elapsed time: {timeit.default_timer() - start:.2f} seconds (scan kernels {timings['kernel_ms']:.1f} ms)")
    logging.info(f"Scanned {total:,} reads: {with_hits:,} with internal primer hits, {n_flagged:,} flagged "
                 f"(rule {args.flag_rule}, inner edit distance {args.inner_edit_distance}, gap {args.junction_gap}); "
                 f"hits per primer: {counts}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
