#!/usr/bin/env python3
"""specimine: mine candidate sequences from partial barcode matches for clustering (reference:
src/specimux/specimine.py, entry cli.py:113-116).

For one specimen's `full/` FASTQ, the partial reads of its forward / reverse barcode (`partial/<pool>/...`) are
kept if they align to one of the specimen's full reads with identity >= --min-identity, where identity is
1 - d / len(full) and d is the HW (infix) edit distance of the full read in the partial read, limited to
k = int(len(full) * (1 - min_identity)).  Every distance is computed on the GPU (smx_mine_best_identity, HIP kernel
smx_mine.hip); there is no CPU path.  The output `<fastq>.mined` holds the mined partial records with the title
`{id}_mined_{type}_{best:.2f} {title} mined_{type} identity={best:.2f}`.

    python -m specimux_amd.specimine --index INDEX.txt --fastq full/POOL/SPECIMEN.fastq [--partial-forward]
        [--no-partial-reverse] [--min-identity 0.85] [--debug]

`mine_specimens(jobs)` mines many specimens in one set of launches (one job = one CLI run)."""
import argparse
import glob
import logging
import os
import re
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .io_utils import SeqRecord, parse_fastq

def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Mine additional candidate sequences from partial matches.")
    parser.add_argument("--index", required=True, help="Path to specimen index file (same as used with specimux)")
    parser.add_argument("--fastq", required=True, help="Path to full match FASTQ file for a specimen")
    parser.add_argument("--partial-forward", action="store_true", default=False,
                        help="Include forward partial matches (default: False)")
    parser.add_argument("--no-partial-reverse", action="store_true", default=False,
                        help="Exclude reverse partial matches (included by default)")
    parser.add_argument("--min-identity", type=float, default=0.85,
                        help="Minimum alignment identity for a match (default: 0.85)")
    parser.add_argument("--debug", action="store_true", help="Enable debug logging")
    return parser


def parse_arguments(argv=None):
    return build_parser().parse_args(argv)


def extract_specimen_id(fastq_path: str) -> str:
    """Specimen id from the FASTQ file name, with or without the legacy `sample_` prefix."""
    filename = os.path.basename(fastq_path)
    match = re.match(r"(?:sample_)?(.+)\.fastq", filename)
    if not match:
        raise ValueError(f"Could not extract specimen ID from filename: {filename}")
    return match.group(1)


def find_barcodes(specimen_id: str, index_file: str) -> Tuple[Optional[str], Optional[str]]:
    """(forward, reverse) barcode of the first index row of the specimen, upper-cased; (None, None) if none."""
    with open(index_file, "r") as fh:
        header = next(fh).strip().split("\t")
        sample_idx = header.index("SampleID") if "SampleID" in header else 0
        fwd_idx = header.index("FwIndex") if "FwIndex" in header else 2
        rev_idx = header.index("RvIndex") if "RvIndex" in header else 4
        need = max(sample_idx, fwd_idx, rev_idx)
        for line in fh:
            fields = line.strip().split("\t")
            if len(fields) > need and fields[sample_idx] == specimen_id:
                return fields[fwd_idx].upper(), fields[rev_idx].upper()
    logging.error(f"Could not find specimen {specimen_id} in index file")
    return None, None


def detect_input_level(fastq_path: str) -> Tuple[str, str, Optional[str]]:
    """(output_root, pool, primer_pair or None) of full/<pool>/X.fastq (pool level) or full/<pool>/<pair>/X.fastq
    (primer-pair level); the first `full` component of the absolute path counts."""
    parts = os.path.abspath(fastq_path).split(os.sep)
    try:
        full_idx = parts.index("full")
    except ValueError:
        raise ValueError(f"Could not find 'full' directory in path: {fastq_path}")
    output_root = os.sep.join(parts[:full_idx])
    remaining = parts[full_idx + 1:-1]
    if len(remaining) == 1:
        return output_root, remaining[0], None
    if len(remaining) == 2:
        return output_root, remaining[0], remaining[1]
    raise ValueError(f"Unexpected path structure: {fastq_path}")


def _find_partial_files(partial_dir: str, fwd_barcode: str, rev_barcode: str, found: Dict[str, List[str]]) -> None:
    """Append the first existing file per barcode (current name, then the legacy `sample_` name) in one directory."""
    if not os.path.isdir(partial_dir):
        return
    for kind, short, barcode in (("forward", "fwd", fwd_barcode), ("reverse", "rev", rev_barcode)):
        if not barcode:
            continue
        for name in (f"barcode_{short}_{barcode}.fastq", f"sample_barcode_{short}_{barcode}.fastq"):
            path = os.path.join(partial_dir, name)
            if os.path.exists(path):
                found[kind].append(path)
                break


def derive_partial_match_filenames(fastq_path: str, fwd_barcode: str, rev_barcode: str) -> Dict[str, List[str]]:
    """{"forward"|"reverse": [partial files]}: partial/<pool>/<pair>/ at primer-pair level, every directory of
    glob(partial/<pool>/*) (in the order glob returns) at pool level.  Empty lists are dropped."""
    found: Dict[str, List[str]] = {"forward": [], "reverse": []}
    output_root, pool, primer_pair = detect_input_level(fastq_path)
    if primer_pair is not None:
        _find_partial_files(os.path.join(output_root, "partial", pool, primer_pair), fwd_barcode, rev_barcode, found)
    else:
        pool_dir = os.path.join(output_root, "partial", pool)
        if os.path.isdir(pool_dir):
            for pp_dir in glob.glob(os.path.join(pool_dir, "*")):
                if os.path.isdir(pp_dir):
                    _find_partial_files(pp_dir, fwd_barcode, rev_barcode, found)
    if fwd_barcode and not found["forward"]:
        logging.warning(f"No forward partial match files found for barcode: {fwd_barcode}")
    if rev_barcode and not found["reverse"]:
        logging.warning(f"No reverse partial match files found for barcode: {rev_barcode}")
    return {k: v for k, v in found.items() if v}


def calculate_identity(alignment_result: Dict, query_length: int) -> float:
    """1 - editDistance / query_length; 0 for a failed alignment (editDistance -1)."""
    d = alignment_result["editDistance"]
    if d == -1:
        return 0
    return 1 - (d / query_length)


def max_distance(full_length: int, min_identity: float) -> int:
    """The edlib limit k of one full read (negative: no limit)."""
    return int(full_length * (1 - min_identity))


def mined_title(record: SeqRecord, partial_type: str, best_identity: float) -> str:
    """Title line (without '@') of a mined record: the id and description the reference sets, joined the way
    Biopython's FASTQ writer joins an id and a description that no longer starts with it."""
    return (f"{record.id}_mined_{partial_type}_{best_identity:.2f} "
            f"{record.description} mined_{partial_type} identity={best_identity:.2f}")


def format_record(title: str, record: SeqRecord) -> str:
    return f"@{title}\n{record.seq}\n+\n{record.quality_string}\n"


def read_fastq(path: str) -> List[SeqRecord]:
    with open(path, "r", encoding="latin-1") as fh:   # one character per byte: the kernel compares bytes
        return list(parse_fastq(fh))


class MineJob:
    """One specimen: its full file, the selected partial files per type and the identity threshold."""

    def __init__(self, fastq: str, partial_files: Dict[str, List[str]], min_identity: float):
        self.fastq = fastq
        self.partial_files = partial_files
        self.min_identity = min_identity
        self.output = f"{fastq}.mined"


def plan_job(index: str, fastq: str, partial_forward: bool = False, no_partial_reverse: bool = False,
             min_identity: float = 0.85) -> MineJob:
    """Everything main() does before mining; exits with status 1 where the reference does."""
    specimen_id = extract_specimen_id(fastq)
    logging.info(f"Processing specimen: {specimen_id}")
    fwd_barcode, rev_barcode = find_barcodes(specimen_id, index)
    if not (fwd_barcode and rev_barcode):
        sys.exit(1)
    logging.info(f"Found barcodes - Forward: {fwd_barcode}, Reverse: {rev_barcode}")
    partial_files = derive_partial_match_filenames(fastq, fwd_barcode, rev_barcode)
    for ptype, files in partial_files.items():
        logging.info(f"Found {len(files)} {ptype} partial match file(s)")
        for f in files:
            logging.debug(f"  - {f}")
    if not partial_forward and "forward" in partial_files:
        del partial_files["forward"]
    if no_partial_reverse and "reverse" in partial_files:
        del partial_files["reverse"]
    if not partial_files:
        logging.error("No partial match files found or selected")
        sys.exit(1)
    return MineJob(fastq, partial_files, min_identity)


def _best_identities(groups, kernel_ms=None) -> List[np.ndarray]:
    """groups: [(full_seqs, partial_seqs, min_identity)] -> per group the best identity of every partial read, all
    groups in one device call (smx_mine_best_identity)."""
    from . import _lib
    lib = _lib.load()
    qparts, tparts, qlens, tlens = [], [], [], []
    jobs = np.zeros(len(groups), dtype=_lib.MINE_JOB_DTYPE)
    k = []
    nq = nt = 0
    for g, (fulls, partials, min_identity) in enumerate(groups):
        jobs[g] = (nq, len(fulls), nt, len(partials), min_identity)
        for s in fulls:
            b = s.encode("latin-1")
            qparts.append(b)
            qlens.append(len(b))
            k.append(max_distance(len(b), min_identity))
        for s in partials:
            b = s.encode("latin-1")
            tparts.append(b)
            tlens.append(len(b))
        nq += len(fulls)
        nt += len(partials)
    qoff = np.zeros(nq + 1, dtype=np.uint64)
    qoff[1:] = np.cumsum(qlens, dtype=np.uint64)
    toff = np.zeros(nt + 1, dtype=np.uint64)
    toff[1:] = np.cumsum(tlens, dtype=np.uint64)
    # a negative k means "no limit"; a limit that does not fit 32 bits is no limit either (d <= len(full) always)
    karr = np.array([min(x, 2**31 - 1) if x >= 0 else -1 for x in k], dtype=np.int32)
    best = np.zeros(max(nt, 1), dtype=np.float64)
    ms = _lib.C.c_float(0.0)
    _lib.check(lib.smx_mine_best_identity(b"".join(qparts), _lib.ptr(qoff), nq, _lib.ptr(karr), b"".join(tparts),
                                          _lib.ptr(toff), nt, _lib.ptr(jobs), len(groups), _lib.ptr(best),
                                          _lib.C.byref(ms)))
    if kernel_ms is not None:
        kernel_ms.append(ms.value)
    out, at = [], 0
    for fulls, partials, _ in groups:
        out.append(best[at:at + len(partials)])
        at += len(partials)
    return out


def mine_specimens(jobs: Sequence[MineJob], kernel_ms=None) -> List[int]:
    """Mine every job in one device call and write each job's `<fastq>.mined`; returns the mined count per job."""
    cache: Dict[str, List[SeqRecord]] = {}

    def records(path):
        if path not in cache:
            cache[path] = read_fastq(path)
        return cache[path]

    plans, groups = [], []
    for job in jobs:
        fulls = records(job.fastq)
        types = []
        if not fulls:
            logging.error(f"No sequences found in full match file: {job.fastq}")
        else:
            logging.info(f"Loaded {len(fulls)} sequences from full match file")
            for ptype, files in job.partial_files.items():
                partials = [r for f in files for r in records(f)]
                types.append((ptype, len(files), partials, len(groups)))
                groups.append(([r.seq for r in fulls], [r.seq for r in partials], job.min_identity))
        plans.append(types)
    best = _best_identities(groups, kernel_ms) if groups else []
    counts = []
    for job, types in zip(jobs, plans):
        out = []
        for ptype, n_files, partials, g in types:
            logging.info(f"Processing {ptype} partial matches from {n_files} file(s)")
            logging.info(f"Found {len(partials)} sequences across all {ptype} partial match files")
            match_count = 0
            for rec, b in zip(partials, best[g]):
                if b > 0:
                    match_count += 1
                    out.append(format_record(mined_title(rec, ptype, float(b)), rec))
            logging.info(f"Matched {match_count}/{len(partials)} sequences from {ptype} partial matches")
        logging.info(f"Found {len(out)} mined sequences")
        with open(job.output, "w", encoding="latin-1") as fh:
            fh.write("".join(out))
        logging.info(f"Wrote {len(out)} sequences to {job.output}")
        counts.append(len(out))
    return counts


def mine_sequences(full_match_file: str, partial_match_files: Dict[str, List[str]],
                   min_identity: float) -> List[Tuple[str, SeqRecord]]:
    """The mined records of one specimen as (title, record) pairs, in the reference's order (types in dict order,
    files in discovery order, records in file order)."""
    fulls = read_fastq(full_match_file)
    if not fulls:
        logging.error(f"No sequences found in full match file: {full_match_file}")
        return []
    logging.info(f"Loaded {len(fulls)} sequences from full match file")
    types = [(t, [r for f in files for r in read_fastq(f)]) for t, files in partial_match_files.items()]
    best = _best_identities([([r.seq for r in fulls], [r.seq for r in p], min_identity) for _, p in types])
    mined = []
    for (ptype, partials), b in zip(types, best):
        n = 0
        for rec, ident in zip(partials, b):
            if ident > 0:
                n += 1
                mined.append((mined_title(rec, ptype, float(ident)), rec))
        logging.info(f"Matched {n}/{len(partials)} sequences from {ptype} partial matches")
    return mined


def main(argv=None):
    args = parse_arguments(argv)
    logging.basicConfig(level=logging.DEBUG if args.debug else logging.INFO,
                        format="%(asctime)s - %(levelname)s - %(message)s")
    job = plan_job(args.index, args.fastq, args.partial_forward, args.no_partial_reverse, args.min_identity)
    mine_specimens([job])


if __name__ == "__main__":
    main()
