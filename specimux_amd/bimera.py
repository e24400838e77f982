#!/usr/bin/env python3
"""specimux-bimera: flag called sequences that are PCR chimeras of two other sequences.  (The reference has no such tool.)

When a well holds two templates, some molecules switch template mid-extension: the product is the left part of one
sequence joined to the right part of another.  It turns up as a minor cluster or a third "haplotype", gets a clean
consensus and a name, and matches nothing.  (specimux-chimera is something else: it finds primers inside a read, which
marks ligated concatemers.)  This tool takes the called sequences of a run -- the --json of specimux-consensus or of
specimux-variants, or their FASTA -- and asks of each: is it a left piece of one more abundant sequence and a right
piece of another?

For a query q of length n, a parent r and e edits, reach(q, r, e) is the longest prefix of q within e edits (unit costs,
exact byte equality after upper-casing, so an N is a mismatch) of some prefix of r, both anchored at their starts; the
right side is the same on the reversed strings.  All of it is computed on the GPU (smx_prefix_reach, HIP kernel
smx_reach.hip, furthest-reaching diagonals), which returns per query, side and e the two furthest-reaching parents;
there is no CPU path and the result is exact.  A parent is eligible for a query if it is another sequence with
size >= ceil(min_parent_ratio * the query's size); the records of --parents (last plate's consensus, a voucher set) are
eligible for every query and are never queries.  With E = max_edits + min_gain:

    d1   the smallest e at which one parent's left reach is n: one parent explains the whole query (else E + 1, ">E")
    d2   the smallest el + er with reach_left(A, el) + reach_right(B, er) >= n for two different parents A and B
         (else E + 1); of several (el, er) the smaller el, then the A of the furthest left reach and the B (other than A)
         of the furthest right reach, the lower index at equal reach
    chimera     d2 <= max_edits and d1 - d2 >= min_gain
    no-parents  no parent is eligible
    ok          otherwise

    python -m specimux_amd.bimera (--consensus C.json | --fasta S.fasta) [--parents P.fasta[.gz]] [--scope specimen|plate]
        [--max-edits 2] [--min-gain 3] [--min-parent-ratio 2.0] [--report T.tsv] [--json J.json] [--clean OUT.fasta]

--scope specimen takes parents from the query's own specimen, where PCR chimeras form; --scope plate takes every sequence
of the run (a parent below the calling threshold in its own well, pooled-PCR protocols).  The parent pool is cut into
pieces under SMX_BIMERA_BUDGET_BYTES (else clusters' budget); the result does not depend on the budget.  One GPU; both
sequences anchored at their starts and ends (no free start offsets); two parents, not three."""
import argparse
import json
import logging
import os
import re
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import calls, clusters, crosstalk, identify, specimine

NONE = 2**64 - 1                           # smx.h: an empty slot
NOT_ELIGIBLE = 2**32 - 1                   # smx.h: the matrix call's value for a target that does not count
MAX_E = 15                                 # SMX_REACH_MAX_E
SLOTS = calls.REACH_SLOTS                  # keys per (query, side, e)
ALWAYS = calls.ALWAYS                      # the weight of a --parents record
Job = Tuple[int, int, int, int]            # (q0, nq, t0, nt): indices into the call's sequence list
COLUMNS = ("name", "specimen", "size", "status", "d1", "d2", "parent_left", "parent_right", "edits_left", "edits_right",
           "break_lo", "break_hi", "length")


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Flag called sequences that are PCR chimeras of two others.")
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("--consensus", help="The --json file of specimux-consensus or specimux-variants")
    source.add_argument("--fasta", help="Their FASTA file: every header carries size=<reads>")
    parser.add_argument("--parents", help="A FASTA of further parents, plain or .gz: eligible for every query, never queries")
    parser.add_argument("--scope", choices=("specimen", "plate"), default="specimen",
                        help="specimen: parents come from the query's own specimen; plate: from the whole run "
                             "(default: specimen)")
    parser.add_argument("--max-edits", type=int, default=2,
                        help="A chimera's two pieces differ from their parents by at most this many edits in all.  A "
                             "choice of the user's, not a measured constant (default: 2)")
    parser.add_argument("--min-gain", type=int, default=3,
                        help="Two parents must explain the sequence with at least this many edits fewer than the best "
                             "single parent.  A choice of the user's, not a measured constant (default: 3)")
    parser.add_argument("--min-parent-ratio", type=float, default=2.0,
                        help="A parent has at least this many times the query's reads.  A choice of the user's, not a "
                             "measured constant (default: 2.0)")
    parser.add_argument("--report", help="Write a TSV: one row per sequence")
    parser.add_argument("--json", help="Write the same table as JSON, with the run summary")
    parser.add_argument("--clean", help="Write a FASTA of every sequence that is not a chimera")
    parser.add_argument("--debug", action="store_true", help="Enable debug logging")
    return parser


# ------------------------------------------------------------------------------------------------ input
class Called:
    """One called sequence: its record name, its specimen, its size in reads, its header line and its sequence."""
    __slots__ = ("name", "specimen", "size", "title", "seq")

    def __init__(self, name: str, specimen: str, size: int, title: str, seq: str):
        self.name, self.specimen, self.size, self.title, self.seq = name, specimen, size, title, seq


def specimen_of(record_name: str) -> str:
    """The specimen a record name stands for: a trailing _c<digits> or _c<digits>_h<digits> removed."""
    return re.sub(r"_c\d+(_h\d+)?$", "", record_name)


def called_from_consensus(path: str) -> List[Called]:
    """The clusters (or haplotypes) with a consensus of a --json file, in file order."""
    refs = crosstalk.refs_from_consensus(path, [])
    with open(path, "r", encoding="latin-1") as fh:
        doc = json.load(fh)
    sizes = [c["size"] for spec in doc.get("specimens", []) for c in spec.get("clusters", []) if c.get("consensus")]
    out = []
    for ref, size in zip(refs, sizes):
        if not isinstance(size, int) or size < 0:
            raise ValueError(f"{path}: record {ref.name!r} has no usable size")
        out.append(Called(ref.name, ref.specimen, size, f"{ref.name} size={size}", ref.seq.upper()))
    return out


def called_from_fasta(path: str) -> List[Called]:
    out = []
    for rec in identify.read_fasta(path):
        m = re.search(r"(?:^|\s)size=(\d+)(?:\s|$)", rec.title)
        if not m:
            raise ValueError(f"{path}: record {rec.ref!r} has no size=<reads> in its header")
        out.append(Called(rec.ref, specimen_of(rec.ref), int(m.group(1)), rec.title, rec.seq))
    return out


# ------------------------------------------------------------------------------------------------ the device call
reach = calls.prefix_reach
reach_matrix = calls.prefix_reach_matrix


def pack_key(reach_: int, target: int) -> int:
    return ((0xFFFFFFFF - reach_) << 32) | target


def unpack_key(key: int) -> Tuple[int, int]:
    """(reach, target index in the call's sequence list) of a key."""
    key = int(key)
    return 0xFFFFFFFF - (key >> 32), key & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ the rule
def need_of(size: int, ratio_permille: int) -> int:
    """ceil(min_parent_ratio * size), in integers."""
    return (ratio_permille * size + 999) // 1000


class Verdict:
    __slots__ = ("status", "d1", "d2", "left", "right", "el", "er", "lo", "hi")

    def __init__(self):
        self.status, self.d1, self.d2 = "ok", 0, 0
        self.left = self.right = self.el = self.er = self.lo = self.hi = None


Best = List[List[List[Tuple[int, int]]]]   # [side][e] -> up to two (reach, parent) in key order


def classify(n: int, best: Best, E: int, max_edits: int, min_gain: int) -> Verdict:
    """The verdict on a query of length n from its two furthest-reaching parents per side and e."""
    v = Verdict()
    v.d1 = v.d2 = E + 1
    if not best[0][0]:
        v.status = "no-parents"
        return v
    for e in range(E + 1):
        if best[0][e][0][0] == n:
            v.d1 = e
            break
    for total in range(E + 1):                     # el + er up to E is enough: E + 1 says "none"
        for el in range(total + 1):
            er = total - el
            pair = _best_pair(best[0][el], best[1][er], n)
            if pair:
                (rl, a), (rr, b) = pair
                v.d2, v.left, v.right, v.el, v.er, v.lo, v.hi = total, a, b, el, er, n - rr, rl
                break
        if v.left is not None:
            break
    if v.d2 <= max_edits and v.d1 - v.d2 >= min_gain:
        v.status = "chimera"
    return v


def _best_pair(left: Sequence[Tuple[int, int]], right: Sequence[Tuple[int, int]], n: int):
    """The first pair (A, B), A != B, in the order (left key, right key) with reach_left(A) + reach_right(B) >= n, among
    ALL eligible parents -- found from the two best of each side: if the best A and the best B differ they decide; if
    they are one parent, only (A1, B2) and (A2, B1) can still do, every other pair reaches no further than both."""
    for a in left:
        for b in right:
            if a[1] != b[1]:
                if a[0] + b[0] >= n:
                    return a, b
                break                              # A's best partner fails: so does every other partner of A
    return None


# ------------------------------------------------------------------------------------------------ one run
def budget_bytes() -> int:
    env = os.environ.get("SMX_BIMERA_BUDGET_BYTES")
    return int(env) if env else clusters.budget_bytes()


def _merge(best: List[Best], keys: np.ndarray, rows: Sequence[int], E: int, to_global: Callable[[int], int]):
    """The keys of one call (rows[i] = the query of output row i) into the per-query lists, target indices made global."""
    per = 2 * (E + 1) * SLOTS
    for i, q in enumerate(rows):
        row = keys[i * per:(i + 1) * per]
        for side in range(2):
            for e in range(E + 1):
                at = (side * (E + 1) + e) * SLOTS
                for key in row[at:at + SLOTS]:
                    if int(key) == NONE:
                        break
                    r, t = unpack_key(key)
                    best[q][side][e].append((r, to_global(t)))


def bimera(called: Sequence[Called], parents: Sequence[identify.Record] = (), scope: str = "specimen", max_edits: int = 2,
           min_gain: int = 3, min_parent_ratio: float = 2.0, budget: Optional[int] = None, reach_fn: Callable = reach,
           kernel_ms: Optional[list] = None) -> Tuple[List[Verdict], Dict]:
    """The verdict on every called sequence, in the order given, and the run summary.  A parent is named by its index:
    0 .. len(called) - 1 are the called sequences, len(called) + i is parents[i]."""
    if max_edits < 0 or min_gain < 0 or max_edits + min_gain > MAX_E:
        raise ValueError(f"--max-edits {max_edits} + --min-gain {min_gain} outside 0..{MAX_E}")
    if not min_parent_ratio >= 0.0:
        raise ValueError(f"--min-parent-ratio {min_parent_ratio} is negative")
    for c in called:
        if not c.seq:
            raise ValueError(f"record {c.name!r} has no sequence")
    E = max_edits + min_gain
    budget = budget if budget is not None else budget_bytes()
    ratio = int(round(min_parent_ratio * 1000))
    N = len(called)
    # the run's sequences grouped by specimen (first appearance), so that a specimen is one index range
    first: Dict[str, int] = {}
    for i, c in enumerate(called):
        first.setdefault(c.specimen, i)
    order = sorted(range(N), key=lambda i: (first[called[i].specimen], i)) if scope == "specimen" else list(range(N))
    seqs = [called[i].seq.encode("latin-1") for i in order]
    weights = [min(called[i].size, ALWAYS - 1) for i in order]
    needs = [min(need_of(called[i].size, ratio), ALWAYS) for i in order]
    if scope == "plate":
        jobs = [(0, N, 0, N)] if N else []
    else:
        jobs, at = [], 0
        while at < N:
            end = at
            while end < N and called[order[end]].specimen == called[order[at]].specimen:
                end += 1
            jobs.append((at, end - at, at, end - at))
            at = end
    best: List[Best] = [[[[] for _ in range(E + 1)] for _ in range(2)] for _ in range(N)]
    summary = {"sequences": N, "parents": len(parents), "scope": scope, "max_edits": max_edits, "min_gain": min_gain,
               "min_parent_ratio": min_parent_ratio, "chimera": 0, "ok": 0, "no-parents": 0, "device_calls": 0}
    if N:
        keys = reach_fn(seqs, weights, needs, jobs, E, kernel_ms)
        summary["device_calls"] += 1
        _merge(best, keys, order, E, lambda t: order[t])
    pool = [p.seq.encode("latin-1") for p in parents]
    pieces = identify.plan_pieces([len(s) for s in pool], max(1, budget - sum(len(s) for s in seqs)))
    for lo, hi in pieces if N else []:
        keys = reach_fn(seqs + pool[lo:hi], weights + [ALWAYS] * (hi - lo), needs + [0] * (hi - lo), [(0, N, N, hi - lo)], E,
                        kernel_ms)
        summary["device_calls"] += 1
        _merge(best, keys, order, E, lambda t, lo=lo: N + lo + (t - N))
    verdicts = []
    for q in range(N):
        for side in range(2):
            for e in range(E + 1):                 # the top two of the union: the top two of the pieces' top twos
                best[q][side][e] = sorted(best[q][side][e], key=lambda x: (-x[0], x[1]))[:SLOTS]
        v = classify(len(called[q].seq), best[q], E, max_edits, min_gain)
        summary[v.status] += 1
        verdicts.append(v)
    return verdicts, summary


# ------------------------------------------------------------------------------------------------ outputs
def rows_of(called: Sequence[Called], parents: Sequence[identify.Record], verdicts: Sequence[Verdict], E: int) -> List[Dict]:
    def name(i):
        return "-" if i is None else called[i].name if i < len(called) else parents[i - len(called)].ref

    def num(x):
        return "-" if x is None else x

    def edits(d):
        return f">{E}" if d > E else d

    return [{"name": c.name, "specimen": c.specimen, "size": c.size, "status": v.status, "d1": edits(v.d1), "d2": edits(v.d2),
             "parent_left": name(v.left), "parent_right": name(v.right), "edits_left": num(v.el), "edits_right": num(v.er),
             "break_lo": num(v.lo), "break_hi": num(v.hi), "length": len(c.seq)} for c, v in zip(called, verdicts)]


def tsv_text(rows: Sequence[Dict]) -> str:
    return "\n".join(["\t".join(COLUMNS)] + ["\t".join(str(r[c]) for c in COLUMNS) for r in rows]) + "\n"


def json_text(rows: Sequence[Dict], summary: Dict) -> str:
    return json.dumps({"summary": summary, "sequences": list(rows)}, indent=1) + "\n"


def clean_text(called: Sequence[Called], verdicts: Sequence[Verdict]) -> str:
    return "".join(f">{c.title}\n{c.seq}\n" for c, v in zip(called, verdicts) if v.status != "chimera")


def summary_line(summary: Dict) -> str:
    return (f"Checked {summary['sequences']} sequence(s) against their {summary['scope']} and {summary['parents']} further "
            f"parent(s) in {summary['device_calls']} device call(s): {summary['chimera']} chimera(s), {summary['ok']} ok, "
            f"{summary['no-parents']} without parents")


def run(args, reach_fn: Callable = reach, kernel_ms: Optional[list] = None) -> int:
    """Everything main() does after parsing; returns the exit status (1 only if the input cannot be read)."""
    try:
        called = called_from_consensus(args.consensus) if args.consensus else called_from_fasta(args.fasta)
        parents = identify.read_fasta(args.parents) if args.parents else []
    except (OSError, ValueError, KeyError, TypeError) as e:
        logging.error(f"Could not read the input: {e}")
        return 1
    verdicts, summary = bimera(called, parents, args.scope, args.max_edits, args.min_gain, args.min_parent_ratio,
                               reach_fn=reach_fn, kernel_ms=kernel_ms)
    logging.info(summary_line(summary))
    rows = rows_of(called, parents, verdicts, args.max_edits + args.min_gain)
    specimine.write_texts(((args.report, lambda: tsv_text(rows)), (args.json, lambda: json_text(rows, summary)),
                           (args.clean, lambda: clean_text(called, verdicts))))
    return 0


def main(argv=None):
    specimine.tool_main(build_parser, run, argv, value_error_status=2)


if __name__ == "__main__":
    main()
