"""The tree algorithm and the tool without a GPU: the numpy twin of smx_nj (tests/tree_utils.py) against neighbour joining
in exact fractions, on additive trees, on the matrices whose every Q ties, and on the ladder matrix that makes double
arithmetic round; then specimux_amd.tree end to end with the twin in place of the two device calls."""
import json
import random
from fractions import Fraction

import numpy as np
import pytest

import tree_utils as U
from specimux_amd import tree


def as_fractions(res):
    merges, last, last_d = res
    return ([(int(m["a"]), int(m["b"]), int(m["n_active"]), Fraction(float(m["d"])), Fraction(float(m["ra"])),
              Fraction(float(m["rb"]))) for m in merges], [int(x) for x in last], [Fraction(float(x)) for x in last_d])


# ------------------------------------------------------------------------------------------------ the algorithm
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 6, 7, 12, 25, 40])
def test_the_twin_is_exact_neighbour_joining_on_small_integers(n):
    """Entries 1..3000, n <= 40: every recorded value has few fractional bits, double arithmetic is exact, and the twin
    must agree with the fractions in pairs, order and every value."""
    rng = random.Random(100 + n)
    for _ in range(3):
        D = U.random_matrix(rng, n)
        got = as_fractions(U.nj_reference(D))
        want = U.nj_exact(D)
        assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
        assert U.same_records(U.nj_scalar(D)[:3], U.nj_reference(D))


@pytest.mark.parametrize("n", [4, 5, 6, 7, 8, 16, 33, 64, 65, 129])
def test_additive_trees_come_back(n):
    """The bipartitions are the generating tree's and every branch length is its integer, exactly; none is negative."""
    for seed in (1, 2):
        D, splits = U.additive_matrix(1000 * seed + n, n)
        assert len(splits) == 2 * n - 3
        got = U.splits_of_result(n, *U.nj_reference(D))
        assert got == splits                        # == on floats against integers: exact or unequal
        assert min(got.values()) >= 1


def test_every_q_ties_n6_by_hand():
    """All-equal 7s: every Q ties in every iteration, so the pair is always the slots (0, 1); slot 1 receives the last
    slot's node after each merge.  Worked by hand from the issue's six steps."""
    merges, last, last_d = U.nj_reference(U.constant_matrix(6, 7))
    assert [tuple(m) for m in merges.tolist()] == [(0, 1, 6, 0, 7.0, 35.0, 35.0), (6, 5, 5, 0, 3.5, 14.0, 24.5),
                                                   (7, 4, 4, 0, 3.5, 10.5, 17.5)]
    assert last.tolist() == [8, 3, 2] and last_d.tolist() == [3.5, 3.5, 7.0]
    merges, last, last_d = U.nj_reference(U.constant_matrix(6, 0))
    assert [tuple(m) for m in merges.tolist()] == [(0, 1, 6, 0, 0.0, 0.0, 0.0), (6, 5, 5, 0, 0.0, 0.0, 0.0), (7, 4, 4, 0, 0.0, 0.0, 0.0)]
    assert last.tolist() == [8, 3, 2] and last_d.tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("value", [0, 7, 2**31 - 1])
@pytest.mark.parametrize("n", [4, 5, 7, 20, 65])
def test_every_q_ties(n, value):
    """The order the tie rule predicts: merge 0 joins the tips 0 and 1, merge t the node of merge t - 1 (slot 0) and the
    tip n - t (slot 1, moved there from the last slot); the tips 3 and 2 remain beside the last node."""
    merges, last, last_d = U.nj_reference(U.constant_matrix(n, value))
    assert [(int(m["a"]), int(m["b"]), int(m["n_active"])) for m in merges] == \
        [(0, 1, n)] + [(n + t - 1, n - t, n - t) for t in range(1, n - 3)]
    assert last.tolist() == [2 * n - 4, 3, 2]
    assert float(merges[0]["ra"]) == float((n - 1) * value)          # the integer row sum, converted once


def test_the_ladder_rounds():
    """D[i][j] = 3 max(i, j) + 1 + (i + j) % 2 at n = 80: double arithmetic is not exact on it, so the twin's records pin
    the order of the operations and the absence of contraction.  A condition on the input, not a tolerance."""
    D = U.ladder_matrix(80)
    assert D[3, 7] == 22 and D[7, 4] == 23 and D[5, 5] == 0 and (D == D.T).all()
    merges, last, last_d, inexact = U.nj_scalar(D, exact_check=True)
    assert inexact >= 1
    assert U.same_records((merges, last, last_d), U.nj_reference(D))
    exact = U.nj_exact(D)                           # and the rounded records are not the exact ones
    assert as_fractions((merges, last, last_d)) != exact


# ------------------------------------------------------------------------------------------------ the tool
def test_the_distance_rule_by_hand():
    seqs = [b"ACGTACGTAC", b"ACGTACGTAA", b"T" * 20]
    ks = tree.limits_of(seqs, 0.30)
    assert ks == [3, 3, 6]
    edits = U.edits_twin(seqs, ks)
    assert edits.tolist() == [1, -1, -1]            # 18 edits to the 20 Ts: above max(3, 6)
    D, above = tree.tree_distances(seqs, ks, edits)
    assert D.tolist() == [1 * 10000 // 10, 7 * 10000 // 20, 7 * 10000 // 20] and above == 2 and D.dtype == np.int32
    # the limit is the longer sequence's, the divisor the longer length; integers, floored
    D, above = tree.tree_distances([b"A" * 7, b"A" * 9, b"A" * 3], [2, 5, 0], np.array([2, -1, 6], dtype=np.int32))
    assert D.tolist() == [2 * 10000 // 9, 3 * 10000 // 7, 6 * 10000 // 9] and above == 1
    assert tree.tree_distances([], [], np.zeros(0, dtype=np.int32))[0].size == 0


def test_labels():
    assert tree.sanitise("a b(c):d;e[f]'g,h\ti") == "a_b_c__d_e_f__g_h_i"
    assert tree.labels_of(["s1", "s 2", "s3"], {"s1": "Genus species;x", "s3": "R(1)"}) == ["s1|Genus_species_x", "s_2", "s3|R_1_"]


def test_nearest_tips():
    D = np.array([[0, 5, 2, 9], [5, 0, 2, 1], [2, 2, 0, 7], [9, 1, 7, 0]])
    who, dist = tree.nearest_tips(U.tri_of(D), 4)
    assert who.tolist() == [2, 3, 0, 1] and dist.tolist() == [2, 1, 2, 1]          # tip 2: 0 and 1 tie, the lower index
    who, dist = tree.nearest_tips(np.zeros(0, dtype=np.int32), 1)
    assert who.tolist() == [-1] and dist.tolist() == [-1]


def test_no_negative():
    rng = random.Random(7)
    for _ in range(200):
        D = U.random_matrix(rng, 6, 1, 40)
        res = U.nj_reference(D)
        plain = tree.Tree(6, *res)
        if plain.negative and any(plain.length[int(m[f])] < 0 for m in res[0] for f in ("a", "b")):
            break
    else:
        pytest.fail("no matrix with a negative child length")
    fixed = tree.Tree(6, *res, no_negative=True)
    assert fixed.negative == plain.negative and min(fixed.length) >= 0.0
    for m in res[0]:
        a, b = int(m["a"]), int(m["b"])
        assert fixed.length[a] + fixed.length[b] == plain.length[a] + plain.length[b]   # the sibling took the difference
        if plain.length[a] < 0:
            assert fixed.length[a] == 0.0 and fixed.length[b] == plain.length[a] + plain.length[b]
    assert "-" not in fixed.newick([f"t{i}" for i in range(6)])
    assert "-" in plain.newick([f"t{i}" for i in range(6)])


def run_tool(tmp_path, names, seqs, tag, extra=(), **fns):
    fasta = tmp_path / f"{tag}.fasta"
    fasta.write_text(U.fasta_text(names, seqs))
    out = {k: tmp_path / f"{tag}.{k}" for k in ("newick", "report", "json")}
    argv = ["--fasta", str(fasta), "--newick", str(out["newick"]), "--report", str(out["report"]), "--json", str(out["json"])]
    args = tree.build_parser().parse_args(argv + list(extra))
    assert tree.run(args, **fns) == 0
    return {k: p.read_bytes() for k, p in out.items()}


def test_the_tool_end_to_end_with_the_twin(tmp_path):
    names, seqs = U.synthetic_plate()
    ident = tmp_path / "identify.json"
    ident.write_text(json.dumps({"queries": [{"query": "g1_s0", "status": "unique", "hits": [{"rank": 1, "ref": "Apis mellifera"}, {"rank": 2, "ref": "x"}]},
                                             {"query": "g2_s3", "status": "none", "hits": []}]}))
    got = run_tool(tmp_path, names, seqs, "plate", ["--identify", str(ident)], edits_fn=U.edits_twin, nj_fn=U.nj_twin)
    labels = [n if n != "g1_s0" else "g1_s0|Apis_mellifera" for n in names]
    text = got["newick"].decode()
    assert text.endswith(");\n") and text.count(",") == len(names) - 1
    splits = U.read_newick(text)
    assert len(splits) == 2 * len(names) - 3
    first = labels[0]
    for g in range(3):                              # three groups of near-identical sequences: three clades
        clade = frozenset(lab for lab in labels if lab.startswith(f"g{g}_"))
        assert (frozenset(labels) - clade if first in clade else clade) in splits, g
    assert all(len(str(v).split(".")[-1]) <= 6 for v in splits.values())
    rows = [line.split("\t") for line in got["report"].decode().splitlines()]
    assert rows[0] == list(tree.COLUMNS) and [r[0] for r in rows[1:]] == names and [r[1] for r in rows[1:]] == labels
    for r in rows[1:]:
        assert r[4][:2] == r[0][:2] and r[4] != r[0]              # the nearest tip is of the tip's own group
        assert r[3] in names or r[3].isdigit()
    doc = json.loads(got["json"])
    assert doc["summary"]["sequences"] == 12 and doc["summary"]["merges"] == 9 and doc["summary"]["labelled"] == 1
    assert doc["summary"]["pairs"] == 66 and doc["summary"]["pairs_above_limit"] == 48      # every pair of two groups
    assert [m["node"] for m in doc["merges"]] == list(range(12, 21)) and len(doc["last"]["nodes"]) == 3
    # the record's values are the twin's, digit for digit
    merges, last, last_d = U.nj_twin(tree.tree_distances([s.encode() for s in seqs], tree.limits_of([s.encode() for s in seqs], 0.30),
                                                         U.edits_twin([s.encode() for s in seqs], tree.limits_of([s.encode() for s in seqs], 0.30)))[0], 12)
    assert [m["d"] for m in doc["merges"]] == [float(x) for x in merges["d"]] and doc["last"]["nodes"] == last.tolist()


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_the_tool_on_fewer_than_four_sequences(tmp_path, n):
    names, seqs = U.synthetic_plate(per_group=1)
    got = run_tool(tmp_path, names[:n], seqs[:n], f"few{n}", edits_fn=U.edits_twin, nj_fn=U.nj_twin)
    text = got["newick"].decode()
    assert text == ";\n" if n == 0 else text.count(":") == n and text.count(",") == n - 1
    assert len(got["report"].decode().splitlines()) == n + 1


def test_the_tool_reads_a_consensus_json(tmp_path):
    names, seqs = U.synthetic_plate(groups=2, per_group=3)
    clusters = [{"name": n, "size": 10 + i, "consensus": s} for i, (n, s) in enumerate(zip(names, seqs))]
    src = tmp_path / "consensus.json"
    src.write_text(json.dumps({"specimens": [{"specimen": "/run/full/W1.fastq", "clusters": clusters[:4]},
                                             {"specimen": "/run/full/W2.fastq", "clusters": clusters[4:] + [{"name": "x", "size": 3, "consensus": ""}]}]}))
    out = tmp_path / "c.nwk"
    args = tree.build_parser().parse_args(["--consensus", str(src), "--newick", str(out)])
    assert tree.run(args, edits_fn=U.edits_twin, nj_fn=U.nj_twin) == 0
    from_fasta = run_tool(tmp_path, names, seqs, "same", edits_fn=U.edits_twin, nj_fn=U.nj_twin)
    assert out.read_bytes() == from_fasta["newick"]
    args = tree.build_parser().parse_args(["--consensus", str(tmp_path / "missing.json")])
    assert tree.run(args, edits_fn=U.edits_twin, nj_fn=U.nj_twin) == 1


def test_duplicate_names_are_an_error(tmp_path):
    fasta = tmp_path / "dup.fasta"
    fasta.write_text(">a\nACGT\n>b\nACGA\n>a\nACGG\n")
    args = tree.build_parser().parse_args(["--fasta", str(fasta)])
    with pytest.raises(ValueError, match="duplicate sequence name 'a'"):
        tree.run(args, edits_fn=U.edits_twin, nj_fn=U.nj_twin)
