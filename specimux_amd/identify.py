#!/usr/bin/env python3
"""specimux-identify: name each consensus sequence of a run from a reference FASTA.  (The reference has no such tool.)

Every query (a consensus of specimux-consensus, or any FASTA record) is compared with every record of a local reference
FASTA -- UNITE, a lab's own voucher sequences, the last plate's consensus file -- and keeps its best few.  The alignment
is semi-global: of a (query, ref) pair the shorter sequence is the pattern and the longer the text, the query at equal
length, and d = HW(pattern in text), the infix edit distance of specimine, limited to
k[pattern] = int(len(pattern) * (1 - min_identity)).  So a primer-to-primer amplicon finds a trimmed database record
inside itself, and finds itself inside an untrimmed GenBank record.  A pair counts only if
len(pattern) >= min_coverage * len(text).  All of it happens on the GPU (smx_best_hits, HIP kernel smx_hits.hip), which
returns per query its K best refs as integer keys (edit fraction, edits, ref index); there is no CPU path, no k-mer screen,
and the result is exact.  Bytes are compared as they are after upper-casing: an N in a ref is a mismatch.

    python -m specimux_amd.identify (--consensus C.json | --fasta QUERIES.fasta) --db REFS.fasta[.gz]
        [--min-identity 0.90] [--top 5] [--min-coverage 0.5] [--strand both|plus] [--report T.tsv] [--json J.json]

Per query the status is `none` (no hit), `tied` (the second hit has the best hit's edit fraction and edits, and another
ref name) or `unique`.  The database is cut into pieces under SMX_IDENTIFY_BUDGET_BYTES (else clusters' budget); each
device call uploads the queries plus one piece, and the host merges the per-call lists, so the result does not depend
on the budget.  One GPU; edit distance only (no affine gaps, no local alignment); at most 16 hits per query."""
import argparse
import gzip
import json
import logging
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import calls, clusters, crosstalk, specimine

NONE = 2**64 - 1                           # smx.h: an empty slot
MAX_K = 16                                 # SMX_HITS_MAX_K
MAX_TARGETS = 1 << 24                      # targets of one job
Job = Tuple[int, int, int, int]            # (q0, nq, t0, nt): indices into the call's sequence list
COLUMNS = ("query", "status", "rank", "ref", "strand", "identity", "edits", "pattern", "coverage", "title")
_COMPLEMENT = bytes.maketrans(b"ACGTRYKMBDHVSWN", b"TGCAYRMKVHDBSWN")


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Name each consensus sequence from a reference FASTA.")
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("--consensus", help="The --json file of specimux-consensus: every consensus is a query")
    source.add_argument("--fasta", help="A FASTA file of queries")
    parser.add_argument("--db", required=True, help="The reference FASTA, plain or .gz; lines may be wrapped")
    parser.add_argument("--min-identity", type=float, default=0.90,
                        help="A hit has at most int(len(pattern) * (1 - this)) edits.  A choice of the user's, not a "
                             "measured constant (default: 0.90)")
    parser.add_argument("--top", type=int, default=5, help=f"Hits kept per query, 1..{MAX_K} (default: 5)")
    parser.add_argument("--min-coverage", type=float, default=0.5,
                        help="A pair counts only if the shorter sequence has at least this share of the longer one's "
                             "length.  A choice of the user's, not a measured constant (default: 0.5)")
    parser.add_argument("--strand", choices=("both", "plus"), default="both",
                        help="both: every ref also enters reverse-complemented (default: both)")
    parser.add_argument("--report", help="Write a TSV: one row per query and hit")
    parser.add_argument("--json", help="Write the same content as JSON, with the run summary")
    parser.add_argument("--debug", action="store_true", help="Enable debug logging")
    return parser


# ------------------------------------------------------------------------------------------------ input
class Record:
    """One FASTA record: `ref` is its name up to the first blank, `title` the whole header line, `seq` upper-cased."""
    __slots__ = ("ref", "title", "seq")

    def __init__(self, title: str, seq: str):
        words = title.split()
        self.ref, self.title, self.seq = (words[0] if words else ""), title, seq


def read_fasta(path: str) -> List[Record]:
    """The records of a FASTA file, plain or gzip (by content), in file order; records without a sequence are left out."""
    with open(path, "rb") as probe:
        gz = probe.read(2) == b"\x1f\x8b"
    out: List[Record] = []
    title, chunks = None, []

    def flush():
        if title is None:
            return
        seq = "".join(chunks).upper()
        if seq:
            out.append(Record(title, seq))
        else:
            logging.warning(f"{path}: record {title!r} has no sequence; left out")

    with (gzip.open(path, "rt", encoding="latin-1") if gz else open(path, "r", encoding="latin-1")) as fh:
        for line in fh:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                flush()
                title, chunks = line[1:], []
            elif title is not None:
                chunks.append(line.strip())
            elif line.strip():
                raise ValueError(f"{path}: sequence data before the first header line")
    flush()
    return out


def queries_from_consensus(path: str) -> List[Record]:
    return [Record(r.name, r.seq.upper()) for r in crosstalk.refs_from_consensus(path, [])]


def revcomp(seq: bytes) -> bytes:
    return seq.translate(_COMPLEMENT)[::-1]


# ------------------------------------------------------------------------------------------------ the device call
best_hits = calls.best_hits
best_hits_distances = calls.best_hits_distances


def pair_rule(len_q: int, len_t: int, min_cov_permille: int) -> Tuple[bool, bool]:
    """(the query is the pattern, the pair is eligible) of a pair of lengths: the library's integer rule."""
    q_is_pattern = len_q <= len_t
    lp, lt = (len_q, len_t) if q_is_pattern else (len_t, len_q)
    return q_is_pattern, lp * 1000 >= min_cov_permille * lt


def pack_key(d: int, len_pattern: int, target: int) -> int:
    return (((d << 20) // len_pattern) << 43) | (d << 24) | target


def unpack_key(key: int) -> Tuple[int, int, int]:
    """(ppm, d, target index within the job) of a key."""
    key = int(key)
    return key >> 43, (key >> 24) & 0x7FFFF, key & 0xFFFFFF


def best_hits_oracle(seqs: Sequence[bytes], ks: Sequence[int], jobs: Sequence[Job], K: int, min_cov_permille: int,
                     kernel_ms: Optional[list] = None) -> np.ndarray:
    """best_hits() by the suite's oracle (edlib HW semantics, exact byte equality) and a sort, pair by pair on the CPU.
    For tests."""
    from oracle.edlib_semantics import HW, align_c
    texts = [s.decode("latin-1") for s in seqs]
    rows = []
    for q0, nq, t0, nt in jobs:
        for q in range(q0, q0 + nq):
            offers = []
            for t in range(t0, t0 + nt):
                q_is_pattern, eligible = pair_rule(len(texts[q]), len(texts[t]), min_cov_permille)
                if not eligible:
                    continue
                p, x = (q, t) if q_is_pattern else (t, q)
                d = align_c(texts[p], texts[x], HW, ks[p], iupac=False)["editDistance"]
                if d >= 0:
                    offers.append(pack_key(d, len(texts[p]), t - t0))
            offers.sort()
            rows.append((offers + [NONE] * K)[:K])
    return np.array(rows, dtype=np.uint64).reshape(-1)


# ------------------------------------------------------------------------------------------------ one run
class Hit:
    __slots__ = ("ppm", "edits", "record", "strand", "len_pattern", "len_text", "pattern")

    def __init__(self, ppm: int, edits: int, record: int, strand: int, len_query: int, len_ref: int):
        self.ppm, self.edits, self.record, self.strand = ppm, edits, record, strand
        q_is_pattern = len_query <= len_ref
        self.pattern = "query" if q_is_pattern else "ref"
        self.len_pattern, self.len_text = (len_query, len_ref) if q_is_pattern else (len_ref, len_query)

    def order(self) -> Tuple[int, int, int, int]:
        return self.ppm, self.edits, self.record, self.strand


class QueryResult:
    def __init__(self, name: str):
        self.name, self.hits, self.status = name, [], "none"


def budget_bytes() -> int:
    env = os.environ.get("SMX_IDENTIFY_BUDGET_BYTES")
    return int(env) if env else clusters.budget_bytes()


def plan_pieces(entry_bytes: Sequence[int], room: int) -> List[Tuple[int, int]]:
    """Cut the database entries, in order, into pieces [lo, hi) of at most `room` bytes and 2^24 entries; an entry that
    alone exceeds the room gets a piece of its own."""
    pieces, lo, cost = [], 0, 0
    for i, b in enumerate(entry_bytes):
        if i > lo and (cost + b > room or i - lo >= MAX_TARGETS):
            pieces.append((lo, i))
            lo, cost = i, 0
        cost += b
    if lo < len(entry_bytes):
        pieces.append((lo, len(entry_bytes)))
    return pieces


def status_of(hits: Sequence[Hit], db: Sequence[Record]) -> str:
    if not hits:
        return "none"
    if len(hits) > 1 and (hits[1].ppm, hits[1].edits) == (hits[0].ppm, hits[0].edits) and db[hits[1].record].ref != db[hits[0].record].ref:
        return "tied"
    return "unique"


def identify(queries: Sequence[Record], db: Sequence[Record], min_identity: float = 0.90, top: int = 5,
             min_coverage: float = 0.5, strand: str = "both", budget: Optional[int] = None, hits_fn: Callable = best_hits,
             kernel_ms: Optional[list] = None) -> Tuple[List[QueryResult], Dict]:
    """The `top` best records of `db` for every query.  Returns the results in query order and the run summary."""
    if not 1 <= top <= MAX_K:
        raise ValueError(f"--top {top} outside 1..{MAX_K}")
    if not 0.0 <= min_coverage <= 1.0:
        raise ValueError(f"--min-coverage {min_coverage} outside 0..1")
    budget = budget if budget is not None else budget_bytes()
    cov = int(round(min_coverage * 1000))
    K = min(MAX_K, max(top, 2))                    # the status looks at the second hit
    q_seqs = [q.seq.encode("latin-1") for q in queries]
    q_ks = [specimine.max_distance(len(s), min_identity) for s in q_seqs]
    # the database entries in (record, strand) order: the order of a target index within a piece is the merge order
    entries: List[Tuple[int, int]] = []
    for i in range(len(db)):
        entries.append((i, 0))
        if strand == "both":
            entries.append((i, 1))
    pieces = plan_pieces([len(db[i].seq) for i, _ in entries], max(1, budget - sum(len(s) for s in q_seqs)))
    results = [QueryResult(q.ref) for q in queries]
    merged: List[List[Hit]] = [[] for _ in queries]
    summary = {"queries": len(queries), "refs": len(db), "unique": 0, "tied": 0, "none": 0, "device_calls": 0}
    for lo, hi in pieces if queries else []:
        seqs, ks = list(q_seqs), list(q_ks)
        for i, rc in entries[lo:hi]:
            s = db[i].seq.encode("latin-1")
            seqs.append(revcomp(s) if rc else s)
            ks.append(specimine.max_distance(len(s), min_identity))
        keys = hits_fn(seqs, ks, [(0, len(queries), len(queries), hi - lo)], K, cov, kernel_ms)
        summary["device_calls"] += 1
        for q in range(len(queries)):
            for key in keys[q * K:(q + 1) * K]:
                if int(key) == NONE:
                    break
                ppm, d, t = unpack_key(key)
                i, rc = entries[lo + t]
                merged[q].append(Hit(ppm, d, i, rc, len(q_seqs[q]), len(db[i].seq)))
    for res, hits in zip(results, merged):
        hits.sort(key=Hit.order)
        res.status = status_of(hits, db)           # from the K best, before the list is cut to --top
        res.hits = hits[:top]
        summary[res.status] += 1
    return results, summary


# ------------------------------------------------------------------------------------------------ outputs
def hit_fields(h: Hit, db: Sequence[Record]) -> Dict:
    return {"ref": db[h.record].ref, "strand": "-" if h.strand else "+", "identity": f"{1 - h.edits / h.len_pattern:.4f}",
            "edits": h.edits, "pattern": h.pattern, "coverage": f"{h.len_pattern / h.len_text:.4f}", "title": db[h.record].title}


def tsv_text(results: Sequence[QueryResult], db: Sequence[Record]) -> str:
    lines = ["\t".join(COLUMNS)]
    for res in results:
        if not res.hits:
            lines.append("\t".join([res.name, res.status] + ["-"] * (len(COLUMNS) - 2)))
        for rank, h in enumerate(res.hits, 1):
            f = hit_fields(h, db)
            lines.append("\t".join(str(x) for x in (res.name, res.status, rank, f["ref"], f["strand"], f["identity"], f["edits"],
                                                    f["pattern"], f["coverage"], f["title"])))
    return "\n".join(lines) + "\n"


def json_text(results: Sequence[QueryResult], db: Sequence[Record], summary: Dict) -> str:
    return json.dumps({"summary": summary,
                       "queries": [{"query": res.name, "status": res.status,
                                    "hits": [dict({"rank": rank}, **hit_fields(h, db)) for rank, h in enumerate(res.hits, 1)]}
                                   for res in results]}, indent=1) + "\n"


def summary_line(summary: Dict) -> str:
    return (f"Compared {summary['queries']} query(ies) with {summary['refs']} ref(s) in {summary['device_calls']} device "
            f"call(s): {summary['unique']} unique, {summary['tied']} tied, {summary['none']} without a hit")


def run(args, hits_fn: Callable = best_hits, kernel_ms: Optional[list] = None) -> int:
    """Everything main() does after parsing; returns the exit status (1 only if the queries or the database cannot be read)."""
    try:
        queries = queries_from_consensus(args.consensus) if args.consensus else read_fasta(args.fasta)
        db = read_fasta(args.db)
    except (OSError, ValueError, KeyError, TypeError) as e:
        logging.error(f"Could not read the input: {e}")
        return 1
    results, summary = identify(queries, db, args.min_identity, args.top, args.min_coverage, args.strand, hits_fn=hits_fn,
                                kernel_ms=kernel_ms)
    logging.info(summary_line(summary))
    specimine.write_texts(((args.report, lambda: tsv_text(results, db)), (args.json, lambda: json_text(results, db, summary))))
    return 0


def main(argv=None):
    specimine.tool_main(build_parser, run, argv, value_error_status=2)


if __name__ == "__main__":
    main()
