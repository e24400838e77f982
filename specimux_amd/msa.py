#!/usr/bin/env python3
"""specimux-msa: a multiple alignment of the called sequences of a run, built along the neighbour-joining tree.  (The
reference has no such tool.)

specimux-tree ends with a tree; everything after it -- a likelihood tree, a look at a suspicious clade in an alignment
viewer, the conserved / variable / informative sites a barcoding report quotes, a bootstrap -- needs aligned columns.  This
tool takes the sequences specimux-tree takes, builds (or reads) the guide tree and aligns progressively along it on the
GPU (smx_msa, HIP kernels smx_msa.hip): every merge of the tree aligns the profiles of its two children by an integer
dynamic programme with traceback, mismatch weight X, gap weight G (linear), and the cost of a merge is the sum of pairs
between the two sides.  Everything is integer and fixed to the last tie-break, so the alignment is the same bytes from run
to run.  There is no CPU path.

    python -m specimux_amd.msa (--consensus C.json | --fasta S.fasta) [--tree TREE.json] [--max-distance 0.30]
        [--mismatch 1] [--gap 1] [--split D --groups-dir DIR] [--fasta-out OUT.fasta] [--order tree|input]
        [--report T.tsv] [--columns C.tsv] [--json J.json]

Guide tree.  --tree is the --json of specimux-tree over the same sequences (the tip names must be the input's names, in
order); without it the tool computes the distances and the join as specimux-tree does.  The unrooted tree becomes a merge
list by one rule: the join's merges in record order, then of the last three nodes the pair with the smallest distance
(ties in the order 01, 02, 12), then that node with the third.

--split D.  Sequences of different orders do not align, so a plate-wide alignment is often noise.  On the tree rooted
at the last merge a group is a maximal node whose tips are pairwise within D (the tree's integer distances, D x 10000);
every group of two or more tips is aligned on its own, along its own subtree, and written to DIR/group_<k>.fasta, k in the
order of the groups' first tips; singletons appear in the report only.

Symbols are A C G T, `other` (any other byte) and the gap.  --report has one row per sequence; `differences` counts the
columns where the row differs from the column's majority symbol, gaps included, ties to the lowest of A C G T other gap.
--columns has one row per column; its class is `conserved` (one symbol), `informative` (at least two symbols in at least
two rows each) or `variable`, gaps counted as a symbol.  Not done here: affine gaps, free end gaps, refinement, sequences
in mixed orientation, bootstrap, rooting."""
import argparse
import json
import logging
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, calls, specimine, tree

SYMBOLS = ("A", "C", "G", "T", "other", "gap")
GAP = ord("-")
REPORT_COLUMNS = ("name", "group", "length", "columns", "gaps", "differences")
COLUMN_COLUMNS = ("group", "column") + SYMBOLS + ("majority", "class")
_CODE = np.full(256, 4, dtype=np.int64)
for _k, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _k
_CODE[GAP] = 5


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="A multiple alignment of the called sequences of a run, along their tree.")
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("--consensus", help="The --json file of specimux-consensus or specimux-variants")
    source.add_argument("--fasta", help="A FASTA file, plain or .gz")
    parser.add_argument("--tree", help="The --json file of specimux-tree over the same sequences: the guide tree")
    parser.add_argument("--max-distance", type=float, default=0.30,
                        help="As in specimux-tree: a sequence's edit limit is int(length * this) (default: 0.30)")
    parser.add_argument("--mismatch", type=int, default=1, help="Weight of a mismatch, 1..1000 (default: 1)")
    parser.add_argument("--gap", type=int, default=1, help="Weight of a gap, 1..1000 (default: 1: with --mismatch 1 a pair's "
                                                         "cost is the edit distance)")
    parser.add_argument("--split", type=float, help="Align groups of sequences pairwise within this distance, each on its own")
    parser.add_argument("--groups-dir", help="With --split: the directory of the groups' aligned FASTA files")
    parser.add_argument("--fasta-out", help="Write the aligned FASTA of the whole run")
    parser.add_argument("--order", choices=("tree", "input"), default="tree",
                        help="Order of the rows of an aligned FASTA: the guide tree's (clades adjacent) or the input's")
    parser.add_argument("--report", help="Write a TSV: one row per sequence")
    parser.add_argument("--columns", help="Write a TSV: one row per column")
    parser.add_argument("--json", help="Write the groups with their merges, lengths and costs, and the summary, as JSON")
    parser.add_argument("--debug", action="store_true", help="Enable debug logging")
    return parser


# ------------------------------------------------------------------------------------------------ the guide tree
def merge_list(n: int, nj_merges, last: Sequence[int], last_d: Sequence[float]) -> List[Tuple[int, int]]:
    """The n - 1 merges of the rooted guide tree from what smx_nj returns for the unrooted one."""
    if n <= 1:
        return []
    if n == 2:
        return [(0, 1)]
    merges = [(int(m["a"]), int(m["b"])) for m in nj_merges]
    d = [float(x) for x in last_d]
    k = min(range(3), key=lambda x: (d[x], x))                 # 01, 02, 12: the first of the smallest
    p, q = ((0, 1), (0, 2), (1, 2))[k]
    third = 3 - p - q
    merges.append((int(last[p]), int(last[q])))
    merges.append((n + len(merges) - 1, int(last[third])))
    return merges


def read_tree(path: str, names: Sequence[str]):
    """(merges, last, last_d) of a specimux-tree --json file, checked against the input's names."""
    with open(path, "r", encoding="latin-1") as fh:
        doc = json.load(fh)
    tips = [str(t["name"]) for t in doc["tips"]]
    if tips != list(names):
        raise ValueError(f"--tree has {len(tips)} tip(s) whose names are not the input's {len(names)} name(s), in order")
    merges = [{"a": int(m["a"]), "b": int(m["b"])} for m in doc["merges"]]
    last = [int(x) for x in doc["last"]["nodes"]] + [0] * 3
    return merges, last[:3], [float(x) for x in doc["last"]["d"]]


def children_of(n: int, merges: Sequence[Tuple[int, int]]) -> Dict[int, Tuple[int, int]]:
    return {n + t: (int(a), int(b)) for t, (a, b) in enumerate(merges)}


def tips_in_tree_order(node: int, n: int, children: Dict[int, Tuple[int, int]]) -> List[int]:
    """The tips under `node`, children in record order; an explicit stack, a ladder is as deep as it has tips."""
    out, stack = [], [node]
    while stack:
        x = stack.pop()
        if x < n:
            out.append(x)
        else:
            a, b = children[x]
            stack.extend((b, a))
    return out


def square_of(tri: np.ndarray, n: int) -> np.ndarray:
    D = np.zeros((n, n), dtype=np.int64)
    at = 0
    for i in range(n - 1):
        D[i, i + 1:] = D[i + 1:, i] = tri[at:at + n - 1 - i]
        at += n - 1 - i
    return D


def split_groups(n: int, merges: Sequence[Tuple[int, int]], tri: np.ndarray, threshold: int) -> List[int]:
    """The nodes of the groups: the maximal nodes whose tips are pairwise within `threshold`; tips where nothing larger is."""
    if n == 0:
        return []
    children = children_of(n, merges)
    D = square_of(tri, n)
    under: List[List[int]] = [[i] for i in range(n)]
    diameter = [0] * n
    for t, (a, b) in enumerate(merges):
        cross = int(D[np.ix_(under[a], under[b])].max())
        under.append(under[a] + under[b])
        diameter.append(max(diameter[a], diameter[b], cross))
    groups, stack = [], [n + len(merges) - 1]
    while stack:
        x = stack.pop()
        if diameter[x] <= threshold:
            groups.append(x)
        else:
            stack.extend(children[x])
    return sorted(groups, key=lambda x: min(under[x]))


def subtree(node: int, n: int, merges: Sequence[Tuple[int, int]]) -> Tuple[List[int], List[Tuple[int, int]]]:
    """The tips under `node` in ascending order and its merges in record order, renumbered: tip k of the list is node k,
    the subtree's merge t makes node len(tips) + t."""
    children = children_of(n, merges)
    tips = sorted(tips_in_tree_order(node, n, children))
    inner, stack = [], [node]
    while stack:
        x = stack.pop()
        if x >= n:
            inner.append(x)
            stack.extend(children[x])
    inner.sort()
    local = {tip: k for k, tip in enumerate(tips)}
    local.update({x: len(tips) + t for t, x in enumerate(inner)})
    return tips, [(local[children[x][0]], local[children[x][1]]) for x in inner]


# ------------------------------------------------------------------------------------------------ columns
def column_counts(rows: np.ndarray) -> np.ndarray:
    """[n_cols, 6]: how many rows hold A, C, G, T, other, gap in each column."""
    codes = _CODE[rows]
    return np.stack([(codes == s).sum(axis=0) for s in range(6)], axis=1).astype(np.int64) if rows.size else np.zeros((0, 6), np.int64)


def column_classes(counts: np.ndarray) -> List[str]:
    present, twice = (counts > 0).sum(axis=1), (counts >= 2).sum(axis=1)
    return ["conserved" if p <= 1 else "informative" if t >= 2 else "variable" for p, t in zip(present, twice)]


def differences(rows: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """Per row the columns where it differs from the majority symbol (the lowest code among the most frequent)."""
    if not rows.size:
        return np.zeros(len(rows), dtype=np.int64)
    return (_CODE[rows] != np.argmax(counts, axis=1)[None, :]).sum(axis=1)


class Group:
    """One aligned group: its index, its tips (input indices, ascending), the rows in that order, the tips in the guide
    tree's order, and what the device call returned."""

    def __init__(self, k: int, tips: List[int], order: List[int], merges, rows: np.ndarray, lens, costs):
        self.k, self.tips, self.order, self.merges, self.rows = k, tips, order, list(merges), rows
        self.lens, self.costs = [int(x) for x in lens], [int(x) for x in costs]
        self.counts = column_counts(rows)
        self.classes = column_classes(self.counts)

    def fasta(self, names: Sequence[str], by: str) -> str:
        where = {tip: r for r, tip in enumerate(self.tips)}
        out = []
        for tip in (self.order if by == "tree" else self.tips):
            text = bytes(self.rows[where[tip]].tolist()).decode("latin-1")
            out.append(f">{names[tip]}\n" + "".join(text[i:i + 80] + "\n" for i in range(0, len(text), 80)))
        return "".join(out)


# ------------------------------------------------------------------------------------------------ outputs
def report_text(names, seqs, groups: Sequence[Group]) -> str:
    lines = ["\t".join(REPORT_COLUMNS)]
    rows = {}
    for g in groups:
        diff = differences(g.rows, g.counts)
        for r, tip in enumerate(g.tips):
            cols = g.rows.shape[1]
            rows[tip] = (names[tip], g.k, len(seqs[tip]), cols, cols - len(seqs[tip]), int(diff[r]))
    lines += ["\t".join(str(x) for x in rows[tip]) for tip in sorted(rows)]
    return "\n".join(lines) + "\n"


def columns_text(groups: Sequence[Group]) -> str:
    lines = ["\t".join(COLUMN_COLUMNS)]
    for g in groups:
        if len(g.tips) < 2:
            continue
        major = np.argmax(g.counts, axis=1) if len(g.counts) else []
        for c, (row, m, cls) in enumerate(zip(g.counts, major, g.classes)):
            lines.append("\t".join(str(x) for x in (g.k, c + 1, *row.tolist(), SYMBOLS[int(m)], cls)))
    return "\n".join(lines) + "\n"


def json_text(names, groups: Sequence[Group], summary: Dict) -> str:
    return json.dumps({"summary": summary,
                       "groups": [{"group": g.k, "tips": [names[t] for t in g.tips], "columns": int(g.rows.shape[1]),
                                   "merges": [[int(a), int(b)] for a, b in g.merges], "lens": g.lens, "costs": g.costs,
                                   "sum_of_pairs": sum(g.costs)} for g in groups]}, indent=1) + "\n"


def summary_line(summary: Dict) -> str:
    return (f"Aligned {summary['sequences']} sequence(s) in {summary['aligned_groups']} group(s) "
            f"({summary['singletons']} singleton(s)): {summary['columns']} column(s), {summary['conserved']} conserved, "
            f"{summary['variable']} variable, {summary['informative']} informative; sum of pairs {summary['sum_of_pairs']}")


def run(args, edits_fn: Callable = tree.device_edits, nj_fn: Callable = calls.nj, msa_fn: Callable = calls.msa,
        kernel_ms: Optional[list] = None) -> int:
    """Everything main() does after parsing; returns the exit status (1 only if the input cannot be read).  edits_fn,
    nj_fn and msa_fn are the three device calls."""
    try:
        names, seqs = tree.read_sequences(args.consensus, args.fasta)
        given = read_tree(args.tree, names) if args.tree else None
    except (OSError, KeyError, TypeError, json.JSONDecodeError) as e:
        logging.error(f"Could not read the input: {e}")
        return 1
    if not 0.0 <= args.max_distance <= 1.0:
        raise ValueError(f"--max-distance {args.max_distance} outside 0..1")
    if not (1 <= args.mismatch <= 1000 and 1 <= args.gap <= 1000):
        raise ValueError("--mismatch and --gap must be 1..1000")
    if args.split is not None and (args.fasta_out or not args.groups_dir or not 0.0 <= args.split <= 1.0):
        raise ValueError("--split D (0..1) goes with --groups-dir and without --fasta-out")
    if args.split is None and args.groups_dir:
        raise ValueError("--groups-dir goes with --split")
    n = len(seqs)
    if n > (_lib.NJ_MAX_N if args.split is not None else _lib.MSA_MAX_N):
        raise ValueError(f"{n} sequences: one alignment holds {_lib.MSA_MAX_N} at the most, one tree {_lib.NJ_MAX_N}")
    tri = None
    if given is None or args.split is not None:
        ks = tree.limits_of(seqs, args.max_distance)
        tri, _ = tree.tree_distances(seqs, ks, edits_fn(seqs, ks, kernel_ms))
    nj_merges, last, last_d = given if given is not None else nj_fn(tri, n, kernel_ms)
    merges = merge_list(n, nj_merges, last, last_d)
    if len(merges) != max(n - 1, 0):
        raise ValueError(f"the guide tree has {len(merges)} merge(s) for {n} sequence(s)")
    children = children_of(n, merges)
    nodes = split_groups(n, merges, tri, int(args.split * tree.SCALE)) if args.split is not None else ([2 * n - 2] if n else [])
    groups: List[Group] = []
    for k, node in enumerate(nodes):
        tips, local = subtree(node, n, merges)
        if len(tips) > _lib.MSA_MAX_N:
            raise ValueError(f"group {k} has {len(tips)} sequences: one alignment holds {_lib.MSA_MAX_N} at the most")
        if len(tips) == 1:
            rows = np.frombuffer(seqs[tips[0]], dtype=np.uint8).reshape(1, -1)
            lens, costs = [], []
        else:
            rows, lens, costs = msa_fn([seqs[t] for t in tips], local, args.mismatch, args.gap, None, kernel_ms)
        groups.append(Group(k, tips, tips_in_tree_order(node, n, children), local, np.asarray(rows), lens, costs))
    aligned = [g for g in groups if len(g.tips) >= 2]
    classes = [c for g in aligned for c in g.classes]
    summary = {"sequences": n, "groups": len(groups), "aligned_groups": len(aligned), "singletons": len(groups) - len(aligned),
               "mismatch": args.mismatch, "gap": args.gap, "split": args.split, "columns": len(classes),
               "conserved": classes.count("conserved"), "variable": classes.count("variable"),
               "informative": classes.count("informative"), "sum_of_pairs": sum(sum(g.costs) for g in groups)}
    logging.info(summary_line(summary))
    outputs = [(args.fasta_out, lambda: "".join(g.fasta(names, args.order) for g in groups)),
               (args.report, lambda: report_text(names, seqs, groups)), (args.columns, lambda: columns_text(groups)),
               (args.json, lambda: json_text(names, groups, summary))]
    if args.split is not None:
        os.makedirs(args.groups_dir, exist_ok=True)
        outputs += [(os.path.join(args.groups_dir, f"group_{g.k}.fasta"), lambda g=g: g.fasta(names, args.order)) for g in aligned]
    specimine.write_texts(outputs)
    return 0


def main(argv=None):
    specimine.tool_main(build_parser, run, argv, value_error_status=2)


if __name__ == "__main__":
    main()
