"""The numpy twin of smx_msa (tests/msa_utils.py) against a brute force, against the project's NW distance and against the
properties the rules promise; then specimux_amd.msa end to end with the twins in place of its three device calls.  No GPU
and no libsmx.so needed."""
import json

import numpy as np
import pytest

import msa_utils as U
import tree_utils as TU
from specimux_amd import consensus, msa

WEIGHTS = [(1, 1), (2, 3), (5, 2)]


def msa_twin(seqs, merges, mismatch=1, gap=1, cap_cols=None, kernel_ms=None):
    """calls.msa on the host."""
    return U.msa_reference(seqs, merges, mismatch, gap)


# ------------------------------------------------------------------------------------------------ the twin
def random_profile(rng, cols: int, tips: int) -> np.ndarray:
    prof = np.zeros((cols, 6), dtype=np.int64)
    for c in range(cols):
        picks = rng.integers(0, 6, size=tips)
        if (picks == 5).all():
            picks[0] = rng.integers(0, 5)          # no column is all gaps
        prof[c] = np.bincount(picks, minlength=6)
    return prof


@pytest.mark.parametrize("X, G", WEIGHTS)
def test_the_twin_is_the_brute_force_s_cost_and_path(X, G):
    rng = np.random.default_rng(X * 100 + G)
    ties = 0
    for _ in range(120):
        na, nb = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        pa, pb = random_profile(rng, int(rng.integers(1, 5)), na), random_profile(rng, int(rng.integers(1, 5)), nb)
        ops, cost = U.merge_profiles(pa, na, pb, nb, X, G)
        want_cost, want_ops, optimal = U.brute_force(pa, na, pb, nb, X, G)
        assert cost == want_cost and ops.tolist() == want_ops.tolist()
        ties += optimal > 1
    assert ties >= 10                                  # cases in which the tie rule had a choice


def test_a_pair_under_unit_weights_costs_the_edit_distance():
    rng = np.random.default_rng(2)
    for _ in range(40):
        a = U.random_seq(rng, int(rng.integers(1, 60)))
        b = U.mutate(rng, a, 0.3) if rng.random() < 0.7 else U.random_seq(rng, int(rng.integers(1, 60)))
        rows, lens, costs = U.msa_reference([a, b], [(0, 1)])
        assert int(costs[0]) == consensus.nw_distance(a.decode(), b.decode())
        assert int(costs[0]) == U.pair_cost_from_rows(rows[0], rows[1], 1, 1)


def check_properties(seqs, merges, X, G):
    rows, lens, costs = U.msa_reference(seqs, merges, X, G)
    n = len(seqs)
    assert rows.shape == (n, int(lens[-1]))
    assert [bytes(r[r != U.GAP].tolist()) for r in rows] == list(seqs)            # a row with the gaps removed is the input
    assert not (rows == U.GAP).all(axis=0).any()                                  # no column is all gaps
    under = U.tips_under(n, merges)
    for t, (a, b) in enumerate(merges):                                           # a merge costs the sum of its pairs
        assert int(costs[t]) == sum(U.pair_cost_from_rows(rows[x], rows[y], X, G) for x in under[a] for y in under[b]), t
    return rows, lens, costs


@pytest.mark.parametrize("X, G", WEIGHTS)
def test_the_four_properties_on_random_trees(X, G):
    rng = np.random.default_rng(7 * X + G)
    for n in range(2, 13):
        seqs = U.family(rng, n, int(rng.integers(15, 50)), 0.25)
        for merges in (U.random_tree(rng, n), U.ladder_tree(n), U.balanced_tree(n)):
            check_properties(seqs, merges, X, G)


def test_other_bytes_and_lower_case():
    """Anything but upper-case A C G T is `other`, and other equals other: n against R costs nothing, a against A does."""
    rows, lens, costs = U.msa_reference([b"ACnGT", b"ACRGT"], [(0, 1)])
    assert costs.tolist() == [0] and rows.tolist() == [list(b"ACnGT"), list(b"ACRGT")]
    rows, lens, costs = U.msa_reference([b"ACaGT", b"ACAGT"], [(0, 1)])
    assert costs.tolist() == [1] and lens.tolist() == [5]
    check_properties([b"ACGTNNacgtRYACGT", b"ACGTNacgGTRACGT", b"ACGNNacgtRYACG"], [(1, 2), (0, 3)], 2, 3)


def test_three_sequences_by_hand():
    """(0, 1) first: ACGT against AGT is one gap, under C (from the end the diagonal is tried first: T, G, then up for C).
    Then the profile A / C- / G / T (two tips) against ACT (one), unit weights.  AC-T costs 1 (the gap under C) + 2 (the
    column G G alone); A-CT costs 1 (the column C- alone, one residue) + 2 (G G against C): a tie, and the walk back, which
    stands at (3, 2) after T, takes the diagonal -- G G against C.  Under (5, 2) the mismatch is dearer: 2 + 10 against
    2 + 4, and C goes under C."""
    rows, lens, costs = U.msa_reference([b"ACGT", b"AGT", b"ACT"], [(0, 1), (3, 2)], 1, 1)
    assert [bytes(r.tolist()) for r in rows] == [b"ACGT", b"A-GT", b"A-CT"]
    assert lens.tolist() == [4, 4] and costs.tolist() == [1, 3]
    rows, lens, costs = U.msa_reference([b"ACGT", b"AGT", b"ACT"], [(0, 1), (3, 2)], 5, 2)
    assert [bytes(r.tolist()) for r in rows] == [b"ACGT", b"A-GT", b"AC-T"] and costs.tolist() == [2, 6]


def test_the_generators_make_valid_trees():
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 7, 33):
        for merges in (U.random_tree(rng, n), U.ladder_tree(n), U.balanced_tree(n)):
            assert len(merges) == n - 1
            seen = set()
            for t, (a, b) in enumerate(merges):
                assert a != b and a < n + t and b < n + t and a not in seen and b not in seen
                seen |= {a, b}


# ------------------------------------------------------------------------------------------------ the tool
def test_the_last_three_nodes_join_by_the_smallest_distance_ties_in_order():
    none = np.zeros(0, dtype=[("a", "<u4"), ("b", "<u4")])
    assert msa.merge_list(3, none, [0, 1, 2], [5.0, 3.0, 4.0]) == [(0, 2), (3, 1)]
    assert msa.merge_list(3, none, [0, 1, 2], [5.0, 4.0, 4.0]) == [(0, 2), (3, 1)]      # 02 before 12
    assert msa.merge_list(3, none, [0, 1, 2], [4.0, 4.0, 4.0]) == [(0, 1), (3, 2)]      # 01 before both
    assert msa.merge_list(3, none, [0, 1, 2], [9.0, 9.0, 4.0]) == [(1, 2), (3, 0)]
    one = np.array([(1, 3)], dtype=[("a", "<u4"), ("b", "<u4")])
    assert msa.merge_list(4, one, [0, 4, 2], [2.0, 2.0, 7.0]) == [(1, 3), (0, 4), (5, 2)]
    assert msa.merge_list(2, none, [0, 1, 0], [3.0, 0.0, 0.0]) == [(0, 1)]
    assert msa.merge_list(1, none, [0, 0, 0], [0.0, 0.0, 0.0]) == [] and msa.merge_list(0, none, [0, 0, 0], [0.0] * 3) == []


def test_the_classes_of_hand_made_columns():
    rows = np.array([list(b"AAAA-A"), list(b"AACA-A"), list(b"ACCT-A"), list(b"ACGN--")], dtype=np.uint8)
    counts = msa.column_counts(rows)
    assert counts.tolist() == [[4, 0, 0, 0, 0, 0], [2, 2, 0, 0, 0, 0], [1, 2, 1, 0, 0, 0], [2, 0, 0, 1, 1, 0],
                               [0, 0, 0, 0, 0, 4], [3, 0, 0, 0, 0, 1]]
    assert msa.column_classes(counts) == ["conserved", "informative", "variable", "variable", "conserved", "variable"]
    # majorities A, A (tie A / C to the lowest), C, A, gap, A
    assert msa.differences(rows, counts).tolist() == [1, 0, 2, 4]


def run_tool(tmp_path, names, seqs, tag, extra=(), **fns):
    fasta = tmp_path / f"{tag}.fasta"
    fasta.write_text(TU.fasta_text(names, seqs))
    out = {k: tmp_path / f"{tag}.{k}" for k in ("report", "columns", "json")}
    argv = ["--fasta", str(fasta), "--report", str(out["report"]), "--columns", str(out["columns"]), "--json", str(out["json"])]
    args = msa.build_parser().parse_args(argv + [str(x) for x in extra])
    assert msa.run(args, **fns) == 0
    got = {k: p.read_bytes() for k, p in out.items()}
    if "--fasta-out" in extra:
        got["fasta"] = (tmp_path / f"{tag}.aln").read_bytes()
    if "--groups-dir" in extra:
        d = tmp_path / f"{tag}.groups"
        got["groups"] = {p.name: p.read_bytes() for p in sorted(d.iterdir())}
    return got


TWINS = dict(edits_fn=TU.edits_twin, nj_fn=TU.nj_twin, msa_fn=msa_twin)


def read_fasta(blob: bytes):
    out = []
    for block in blob.decode().split(">")[1:]:
        head, *lines = block.split("\n")
        assert all(len(x) <= 80 for x in lines)
        out.append((head, "".join(lines)))
    return out


def plate():
    """Three planted groups of four near-identical sequences, interleaved so that input order is not tree order."""
    names, seqs = TU.synthetic_plate(seed=31, groups=3, per_group=4, length=100)
    order = [0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11]
    return [names[i] for i in order], [seqs[i] for i in order]


def test_the_tool_end_to_end_in_both_orders(tmp_path):
    names, seqs = plate()
    by_tree = run_tool(tmp_path, names, seqs, "t", ["--fasta-out", tmp_path / "t.aln"], **TWINS)
    by_input = run_tool(tmp_path, names, seqs, "i", ["--fasta-out", tmp_path / "i.aln", "--order", "input"], **TWINS)
    a, b = read_fasta(by_tree["fasta"]), read_fasta(by_input["fasta"])
    assert [h for h, _ in b] == names and sorted(a) == sorted(b) and [h for h, _ in a] != names
    heads = [h[:2] for h, _ in a]
    # clades are adjacent in tree order; the root may lie inside one of them, which then wraps around the ends
    assert sum(heads[k] != heads[(k + 1) % 12] for k in range(12)) == 3
    assert len({len(s) for _, s in a}) == 1 and [s.replace("-", "") for _, s in b] == seqs
    assert by_tree["report"] == by_input["report"] and by_tree["columns"] == by_input["columns"]
    report = [line.split("\t") for line in by_tree["report"].decode().splitlines()]
    assert report[0] == list(msa.REPORT_COLUMNS) and [r[0] for r in report[1:]] == names
    cols = len(a[0][1])
    assert all(r[1] == "0" and int(r[3]) == cols and int(r[4]) == cols - int(r[2]) for r in report[1:])
    columns = [line.split("\t") for line in by_tree["columns"].decode().splitlines()]
    assert columns[0] == list(msa.COLUMN_COLUMNS) and len(columns) == cols + 1
    assert all(sum(int(x) for x in c[2:8]) == 12 for c in columns[1:])
    doc = json.loads(by_tree["json"])
    assert doc["summary"]["sequences"] == 12 and doc["summary"]["aligned_groups"] == 1 and doc["summary"]["columns"] == cols
    assert doc["summary"]["conserved"] + doc["summary"]["variable"] + doc["summary"]["informative"] == cols
    g, = doc["groups"]
    assert len(g["merges"]) == len(g["lens"]) == len(g["costs"]) == 11 and g["sum_of_pairs"] == sum(g["costs"]) == doc["summary"]["sum_of_pairs"]
    rows = np.array([list(s.encode()) for _, s in b], dtype=np.uint8)
    assert g["sum_of_pairs"] == sum(U.pair_cost_from_rows(rows[x], rows[y], 1, 1) for x in range(12) for y in range(x + 1, 12))


def planted_plate(seed: int = 1, far=(12, 18, 25)):
    """Three groups of four (0..2 substitutions apart) whose founders lie 12, 18 and 25 substitutions from one ancestor of 100
    bases, interleaved.  Chosen so that the join's last three nodes are the three groups: see the second half of the test."""
    import random
    rng = random.Random(seed)
    ancestor = [rng.choice("ACGT") for _ in range(100)]

    def substituted(base, k):
        out = list(base)
        for at in rng.sample(range(100), k):
            out[at] = rng.choice([c for c in "ACGT" if c != out[at]])
        return out
    names, seqs = [], []
    for g in range(3):
        founder = substituted(ancestor, far[g])
        for i in range(4):
            names.append(f"g{g}_s{i}")
            seqs.append("".join(substituted(founder, i % 3)))
    order = [0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11]
    return [names[i] for i in order], [seqs[i] for i in order]


def test_split_finds_the_three_planted_groups(tmp_path):
    names, seqs = planted_plate()
    extra = ["--max-distance", "0.5", "--split", "0.10"]
    got = run_tool(tmp_path, names, seqs, "s", extra + ["--groups-dir", tmp_path / "s.groups"], **TWINS)
    assert sorted(got["groups"]) == ["group_0.fasta", "group_1.fasta", "group_2.fasta"]
    for k in range(3):
        members = read_fasta(got["groups"][f"group_{k}.fasta"])
        assert sorted(h for h, _ in members) == sorted(n for n in names if n.startswith(f"g{k}_"))      # by the first tip: g0, g1, g2
        assert {len(s) for _, s in members} == {100}                                                    # substitutions only: no gaps
    report = [line.split("\t") for line in got["report"].decode().splitlines()[1:]]
    assert [r[0] for r in report] == names and [r[1] for r in report] == [n[1] for n in names]
    doc = json.loads(got["json"])
    assert doc["summary"]["aligned_groups"] == 3 and doc["summary"]["singletons"] == 0
    assert [len(g["merges"]) for g in doc["groups"]] == [3, 3, 3]
    # Known limitation: the groups are nodes of the tree rooted at the join's last merge, and on a
    # plate of unrelated groups the join ends inside one of them, which then comes out in pieces.  Whatever the rooting,
    # every sequence is in exactly one group, the files are the groups of two or more, and singletons are in the report.
    names, seqs = plate()
    got = run_tool(tmp_path, names, seqs, "u", ["--split", "0.10", "--groups-dir", tmp_path / "u.groups"], **TWINS)
    doc = json.loads(got["json"])
    assert sorted(t for g in doc["groups"] for t in g["tips"]) == sorted(names)
    assert all(t[:2] == g["tips"][0][:2] for g in doc["groups"] for t in g["tips"])          # no group mixes planted groups
    assert sorted(got["groups"]) == sorted(f"group_{g['group']}.fasta" for g in doc["groups"] if len(g["tips"]) >= 2)
    assert len(got["report"].decode().splitlines()) == 13


def test_split_refuses_the_whole_run_fasta(tmp_path):
    names, seqs = plate()
    with pytest.raises(ValueError, match="--split"):
        run_tool(tmp_path, names, seqs, "x", ["--split", "0.1", "--groups-dir", tmp_path / "x.groups", "--fasta-out", tmp_path / "x.aln"], **TWINS)
    with pytest.raises(ValueError, match="--split"):
        run_tool(tmp_path, names, seqs, "y", ["--split", "0.1"], **TWINS)


def test_a_given_tree_must_carry_the_input_s_names(tmp_path):
    from specimux_amd import tree
    names, seqs = plate()
    fasta = tmp_path / "in.fasta"
    fasta.write_text(TU.fasta_text(names, seqs))
    tree_json = tmp_path / "tree.json"
    assert tree.run(tree.build_parser().parse_args(["--fasta", str(fasta), "--json", str(tree_json)]),
                    edits_fn=TU.edits_twin, nj_fn=TU.nj_twin) == 0

    def no_call(*args, **kwargs):
        raise AssertionError("the guide tree was given")
    with_tree = run_tool(tmp_path, names, seqs, "w", ["--tree", tree_json, "--fasta-out", tmp_path / "w.aln"],
                         edits_fn=no_call, nj_fn=no_call, msa_fn=msa_twin)
    without = run_tool(tmp_path, names, seqs, "o", ["--fasta-out", tmp_path / "o.aln"], **TWINS)
    assert with_tree == without
    with pytest.raises(ValueError, match="names"):
        run_tool(tmp_path, names[1:] + names[:1], seqs[1:] + seqs[:1], "r", ["--tree", tree_json], **TWINS)
    with pytest.raises(ValueError, match="names"):
        run_tool(tmp_path, names[:-1], seqs[:-1], "q", ["--tree", tree_json], **TWINS)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_the_smallest_runs(tmp_path, n):
    names, seqs = plate()
    got = run_tool(tmp_path, names[:n], seqs[:n], "small", ["--fasta-out", tmp_path / "small.aln"], **TWINS)
    assert [h for h, _ in read_fasta(got["fasta"])].__len__() == n
    assert json.loads(got["json"])["summary"]["sequences"] == n
