#!/usr/bin/env python3
"""specimux-tree: a neighbour-joining tree of all called sequences of a run.  (The reference has no such tool.)

Every other long-read tool here looks at one specimen at a time; this one looks at the plate as a whole: which specimens
carry the same sequence or the same species, which specimen sits in a clade its label does not belong to (a swapped tube, a
misidentified voucher), and where the sequences specimux-identify could not name fall among the named ones.  It takes the
called sequences of a run -- the --json of specimux-consensus or of specimux-variants, or a FASTA -- and writes the tree a
barcoding run is usually delivered with.

Distances.  All pairs are aligned on the GPU (smx_pairs_distances, exact NW edit distances under a band; row blocks
through smx_nearest_distances, the same NW, if that call refuses the size).  Sequence i's limit is
k_i = int(len_i * max_distance), a pair's limit that of its longer sequence; a pair above its limit counts as limit + 1
edits.  The tree's distance is the integer D = edits * 10000 // max(len_i, len_j).

Tree.  The join runs on the GPU (smx_nj, HIP kernels smx_nj.hip): the algorithm is fixed to the last floating-point
operation, so the merges and lengths are the same from run to run.  The device returns the merge records; the branch
lengths follow here, la = d / 2 + (ra - rb) / (2 (n_active - 2)), lb = d - la, and the three-point formula for the
three nodes that remain.  There is no CPU path.

    python -m specimux_amd.tree (--consensus C.json | --fasta S.fasta) [--max-distance 0.30] [--identify I.json]
        [--newick OUT.nwk] [--report T.tsv] [--json J.json] [--no-negative]

--newick is unrooted, a trifurcation at the last three nodes, children in record order, lengths D / 10000 with six
decimals; a tip's label is its name, then `|` and the rank-1 ref of --identify (the --json of specimux-identify) where
there is one; ( ) , : ; [ ] ' and blanks in a label become _.  --no-negative sets a negative child length to 0 and gives
the difference to its sibling (at the trifurcation, where a node has two siblings, it is set to 0 alone).  --report has
one row per tip: its branch length, its sister (a tip's name, or the size of the sister clade) and its nearest other
tip by the distance matrix.  Not done here: rooting, bootstrap support, species groups by a threshold, sequences in
mixed orientation, any other distance."""
import argparse
import json
import logging
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, bimera, calls, clusters, identify, specimine

SCALE = 10000                              # the tree's distances are integers per 10 000 bases
COLUMNS = ("name", "label", "length", "sister", "nearest", "nearest_distance")
UNSAFE = set("(),:;[]'")                   # what a Newick label may not hold, blanks apart


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="A neighbour-joining tree of the called sequences of a run.")
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("--consensus", help="The --json file of specimux-consensus or specimux-variants")
    source.add_argument("--fasta", help="A FASTA file, plain or .gz")
    parser.add_argument("--max-distance", type=float, default=0.30,
                        help="A sequence's edit limit is int(length * this); a pair above the limit of its longer sequence "
                             "counts as limit + 1 edits.  A choice of the user's, not a measured constant (default: 0.30)")
    parser.add_argument("--identify", help="The --json file of specimux-identify: its rank-1 refs are added to the labels")
    parser.add_argument("--newick", help="Write the tree in Newick format")
    parser.add_argument("--report", help="Write a TSV: one row per tip")
    parser.add_argument("--json", help="Write the merges, the lengths and the run summary as JSON")
    parser.add_argument("--no-negative", action="store_true", help="Set negative branch lengths to 0 (the sibling takes the difference)")
    parser.add_argument("--debug", action="store_true", help="Enable debug logging")
    return parser


# ------------------------------------------------------------------------------------------------ input
def read_sequences(consensus: Optional[str], fasta: Optional[str]) -> Tuple[List[str], List[bytes]]:
    """The names and sequences of the run, in file order.  Duplicate names are an error."""
    if consensus:
        records = [(c.name, c.seq) for c in bimera.called_from_consensus(consensus)]
    else:
        records = [(r.ref, r.seq) for r in identify.read_fasta(fasta)]
    names = [name for name, _ in records]
    seen = set()
    for name in names:
        if name in seen:
            raise ValueError(f"duplicate sequence name {name!r}")
        seen.add(name)
    for name, seq in records:
        if not seq:
            raise ValueError(f"record {name!r} has no sequence")
    return names, [seq.upper().encode("latin-1") for _, seq in records]


def identify_refs(path: str) -> Dict[str, str]:
    """query -> the rank-1 ref of a specimux-identify --json file, for the queries with a hit."""
    with open(path, "r", encoding="latin-1") as fh:
        doc = json.load(fh)
    out = {}
    for q in doc.get("queries", []):
        for hit in q.get("hits", []):
            if hit.get("rank") == 1:
                out[q["query"]] = str(hit["ref"])
                break
    return out


def sanitise(label: str) -> str:
    return "".join("_" if ch in UNSAFE or ch.isspace() else ch for ch in label)


def labels_of(names: Sequence[str], refs: Dict[str, str]) -> List[str]:
    return [sanitise(f"{name}|{refs[name]}" if name in refs else name) for name in names]


# ------------------------------------------------------------------------------------------------ distances
def limits_of(seqs: Sequence[bytes], max_distance: float) -> List[int]:
    return [int(len(s) * max_distance) for s in seqs]


def device_edits(seqs: Sequence[bytes], ks: Sequence[int], kernel_ms: Optional[list] = None) -> np.ndarray:
    """The packed upper triangle of NW edit distances (-1 above a pair's limit): one smx_pairs_distances job over all
    sequences, or, if its plan refuses the size, row blocks through smx_nearest_distances."""
    n = len(seqs)
    if n < 2:
        return np.zeros(0, dtype=np.int32)
    try:
        return np.array(calls.pairs_distances(seqs, ks, [(0, n)], kernel_ms)[0], dtype=np.int32)
    except _lib.SmxError as e:
        if e.code != _lib.ERR_UNSUPPORTED:
            raise
        logging.info(f"One pairs job was refused ({e}); using row blocks")
    tri = np.empty(n * (n - 1) // 2, dtype=np.int32)
    rows = max(1, min(n, clusters.budget_bytes() // (4 * n)))
    at = 0
    for r0 in range(0, n - 1, rows):
        nb = min(rows, n - 1 - r0)
        block = calls.nearest_distances(seqs, ks, [0] * n, [(r0, nb, 0, n)], kernel_ms)[0]
        for i in range(nb):
            row = r0 + i
            tri[at:at + n - 1 - row] = block[i, row + 1:]
            at += n - 1 - row
    return tri


def tree_distances(seqs: Sequence[bytes], ks: Sequence[int], edits: np.ndarray) -> Tuple[np.ndarray, int]:
    """The tree's integer distances D = edits * 10000 // max(len_i, len_j) as a packed triangle, a pair reported -1 taken
    as max(k_i, k_j) + 1 edits; and the number of such pairs.  Integers only."""
    n = len(seqs)
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    karr = np.array(ks, dtype=np.int64)
    out = np.empty(n * (n - 1) // 2, dtype=np.int32)
    above, at = 0, 0
    for i in range(n - 1):
        e = np.asarray(edits[at:at + n - 1 - i], dtype=np.int64)
        over = e < 0
        above += int(over.sum())
        e = np.where(over, np.maximum(karr[i], karr[i + 1:]) + 1, e)
        out[at:at + n - 1 - i] = e * SCALE // np.maximum(lens[i], lens[i + 1:])
        at += n - 1 - i
    return out, above


def nearest_tips(tri: np.ndarray, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """Per tip its nearest other tip (the lowest index at equal distance) and that distance; -1 where there is none."""
    who = np.full(n, -1, dtype=np.int64)
    dist = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
    at = 0
    for i in range(n - 1):
        seg = np.asarray(tri[at:at + n - 1 - i], dtype=np.int64)
        at += n - 1 - i
        j = int(np.argmin(seg))
        if seg[j] < dist[i]:                       # the tips before i were offered first: they keep a tie
            who[i], dist[i] = i + 1 + j, seg[j]
        better = seg < dist[i + 1:]
        who[i + 1:][better] = i
        dist[i + 1:][better] = seg[better]
    dist[who < 0] = -1
    return who, dist


# ------------------------------------------------------------------------------------------------ the tree
class Tree:
    """The unrooted tree of n tips: node n + t has the children `children[n + t]` (in record order); `length[x]` is the
    branch above node x; `top` are the nodes of the trifurcation (all the nodes, for n <= 3); `parent[x]` is -1 there."""

    def __init__(self, n: int, merges: np.ndarray, last: Sequence[int], last_d: Sequence[float], no_negative: bool = False):
        self.n = n
        total = n + len(merges)
        self.children: Dict[int, Tuple[int, int]] = {}
        self.length = [0.0] * total
        self.parent = [-1] * total
        self.size = [1] * n + [0] * len(merges)
        self.negative = 0
        for t, m in enumerate(merges):
            a, b, na = int(m["a"]), int(m["b"]), int(m["n_active"])
            d, ra, rb = float(m["d"]), float(m["ra"]), float(m["rb"])
            la = 0.5 * d + (ra - rb) / (2 * (na - 2))
            lb = d - la
            self.negative += (la < 0) + (lb < 0)
            if no_negative:
                if la < 0:
                    la, lb = 0.0, lb + la
                elif lb < 0:
                    la, lb = la + lb, 0.0
            self.children[n + t] = (a, b)
            self.length[a], self.length[b] = la, lb
            self.parent[a] = self.parent[b] = n + t
            self.size[n + t] = self.size[a] + self.size[b]
        self.top = [int(x) for x in last[:min(n, 3)]]
        d01, d02, d12 = (float(x) for x in last_d)
        if n == 2:
            tops = [0.5 * d01, d01 - 0.5 * d01]
        elif n >= 3:
            tops = [0.5 * (d01 + d02 - d12), 0.5 * (d01 + d12 - d02), 0.5 * (d02 + d12 - d01)]
        else:
            tops = [0.0] * n
        for x, length in zip(self.top, tops):
            self.negative += length < 0
            self.length[x] = 0.0 if no_negative and length < 0 else length

    def newick(self, labels: Sequence[str]) -> str:
        def fmt(x):
            s = f"{self.length[x] / SCALE:.6f}"
            return "0.000000" if s == "-0.000000" else s

        out: List[str] = []
        for i, x in enumerate(self.top):           # an explicit stack: a ladder of 16 384 tips is as deep
            if i:
                out.append(",")
            stack: List = [x]
            while stack:
                item = stack.pop()
                if isinstance(item, str):
                    out.append(item)
                elif item < self.n:
                    out.append(f"{labels[item]}:{fmt(item)}")
                else:
                    a, b = self.children[item]
                    out.append("(")
                    stack.extend((f"):{fmt(item)}", b, ",", a))
        if self.n == 0:
            return ";\n"
        return "(" + "".join(out) + ");\n"

    def sister(self, x: int, names: Sequence[str]) -> str:
        """The sister of tip x: a tip's name, or the size of the sister clade (at the trifurcation: of the two others)."""
        p = self.parent[x]
        others = [y for y in (self.children[p] if p >= 0 else self.top) if y != x]
        if not others:
            return "-"
        if len(others) == 1 and others[0] < self.n:
            return names[others[0]]
        return str(sum(self.size[y] for y in others))


# ------------------------------------------------------------------------------------------------ outputs
def rows_of(names, labels, tree: Tree, who, dist) -> List[Dict]:
    return [{"name": names[i], "label": labels[i], "length": f"{tree.length[i] / SCALE:.6f}", "sister": tree.sister(i, names),
             "nearest": names[int(who[i])] if who[i] >= 0 else "-",
             "nearest_distance": f"{int(dist[i]) / SCALE:.4f}" if who[i] >= 0 else "-"} for i in range(tree.n)]


def tsv_text(rows: Sequence[Dict]) -> str:
    return "\n".join(["\t".join(COLUMNS)] + ["\t".join(str(r[c]) for c in COLUMNS) for r in rows]) + "\n"


def json_text(names, labels, merges: np.ndarray, last, last_d, tree: Tree, summary: Dict) -> str:
    n = tree.n
    return json.dumps({"summary": summary,
                       "tips": [{"node": i, "name": names[i], "label": labels[i], "length": tree.length[i]} for i in range(n)],
                       "merges": [{"node": n + t, "a": int(m["a"]), "b": int(m["b"]), "n_active": int(m["n_active"]),
                                   "d": float(m["d"]), "ra": float(m["ra"]), "rb": float(m["rb"]),
                                   "length_a": tree.length[int(m["a"])], "length_b": tree.length[int(m["b"])]}
                                  for t, m in enumerate(merges)],
                       "last": {"nodes": tree.top, "d": [float(x) for x in last_d],
                                "lengths": [tree.length[x] for x in tree.top]}}, indent=1) + "\n"


def summary_line(summary: Dict) -> str:
    return (f"Joined {summary['sequences']} sequence(s) in {summary['merges']} merge(s): {summary['pairs_above_limit']} of "
            f"{summary['pairs']} pair(s) above their limit, {summary['negative_lengths']} negative branch length(s)")


def run(args, edits_fn: Callable = device_edits, nj_fn: Callable = calls.nj, kernel_ms: Optional[list] = None) -> int:
    """Everything main() does after parsing; returns the exit status (1 only if the input cannot be read).  edits_fn and
    nj_fn are the two device calls."""
    try:
        names, seqs = read_sequences(args.consensus, args.fasta)
        refs = identify_refs(args.identify) if args.identify else {}
    except (OSError, KeyError, TypeError, json.JSONDecodeError) as e:
        logging.error(f"Could not read the input: {e}")
        return 1
    if not 0.0 <= args.max_distance <= 1.0:
        raise ValueError(f"--max-distance {args.max_distance} outside 0..1")
    n = len(seqs)
    if n > _lib.NJ_MAX_N:
        raise ValueError(f"{n} sequences: one tree holds {_lib.NJ_MAX_N} at the most")
    labels = labels_of(names, refs)
    ks = limits_of(seqs, args.max_distance)
    tri, above = tree_distances(seqs, ks, edits_fn(seqs, ks, kernel_ms))
    merges, last, last_d = nj_fn(tri, n, kernel_ms)
    tree = Tree(n, merges, last, last_d, args.no_negative)
    summary = {"sequences": n, "pairs": n * (n - 1) // 2, "pairs_above_limit": above, "max_distance": args.max_distance,
               "merges": len(merges), "negative_lengths": int(tree.negative), "no_negative": bool(args.no_negative),
               "labelled": sum(1 for name in names if name in refs)}
    logging.info(summary_line(summary))

    def report():
        return tsv_text(rows_of(names, labels, tree, *nearest_tips(tri, n)))

    specimine.write_texts(((args.newick, lambda: tree.newick(labels)), (args.report, report),
                           (args.json, lambda: json_text(names, labels, merges, last, last_d, tree, summary))))
    return 0


def main(argv=None):
    specimine.tool_main(build_parser, run, argv, value_error_status=2)


if __name__ == "__main__":
    main()
