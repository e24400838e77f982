"""specimux-identify end to end without a GPU: the tool over the synthetic database of tests/identify_utils.py, with
identify.best_hits_oracle (the suite's HW oracle and a sort) in place of the device call.  The planted outcomes are
asserted: pattern = query and pattern = ref, a ref found only reverse-complemented, tied and unique twins, the limit one
edit inside and outside, the coverage bound, a query without a relative; also wrapped and lower-case FASTA, gz input, the
consensus JSON as the query source, and byte-identical reports under three budgets."""
import json
import os

import pytest

from specimux_amd import identify, specimine

import identify_utils as U


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = os.fspath(tmp_path_factory.mktemp("identify"))
    queries, refs = U.build_files(root)
    return root, queries, refs


@pytest.fixture(scope="module")
def base_run(tree, tmp_path_factory):
    """The default run (both strands, coverage 0.5, one piece), shared by the tests that only read it."""
    root, _, _ = tree
    out = os.fspath(tmp_path_factory.mktemp("base"))
    assert identify.run(U.args_for(root, out), hits_fn=identify.best_hits_oracle) == 0
    return U.outputs(out)


def test_planted_outcomes(tree, base_run):
    _, queries, refs = tree
    rows = U.rows_of(base_run["report.tsv"])
    assert list(rows) == list(U.QUERIES)
    first = {q: r[0] for q, r in rows.items()}
    f = first["Q_FLANK"]                           # the ref carries the flanks: the query is the pattern
    assert (f["status"], f["ref"], f["strand"], f["pattern"], f["edits"], f["rank"]) == ("unique", "REF_FLANK", "+", "query", "2", "1")
    assert f["identity"] == f"{1 - 2 / 300:.4f}" and f["coverage"] == f"{300 / 420:.4f}" and f["title"] == "REF_FLANK Fungus flankii voucher 1"
    t = first["Q_TRIM"]                            # the ref is trimmed: the ref is the pattern
    assert (t["status"], t["ref"], t["strand"], t["pattern"], t["edits"]) == ("unique", "REF_TRIM", "+", "ref", "3")
    assert t["identity"] == f"{1 - 3 / 300:.4f}" and t["coverage"] == f"{300 / 420:.4f}"
    r = first["Q_RC"]
    assert (r["status"], r["ref"], r["strand"], r["edits"]) == ("unique", "REF_RC", "-", "1")
    tied = rows["Q_TIED"]                          # two names, one sequence: tied, the earlier record first
    assert [x["status"] for x in tied] == ["tied", "tied"] and {x["ref"] for x in tied} == {"TWIN_A", "TWIN_B"}
    assert [x["edits"] for x in tied] == ["0", "0"] and [x["rank"] for x in tied] == ["1", "2"]
    order = [title.split()[0] for title, _ in refs]
    assert [x["ref"] for x in tied] == sorted(("TWIN_A", "TWIN_B"), key=order.index)
    same = rows["Q_SAME"]                          # one name twice: unique
    assert [x["status"] for x in same] == ["unique", "unique"] and [x["ref"] for x in same] == ["SAME_NAME"] * 2
    assert {x["title"] for x in same} == {"SAME_NAME copy 1", "SAME_NAME copy 2"}
    k = specimine.max_distance(300, U.MIN_IDENTITY)
    lim = rows["Q_LIMIT"]                          # k edits: a hit; k + 1: not
    assert [(x["ref"], x["edits"], x["status"]) for x in lim] == [("LIMIT_IN", str(k), "unique")]
    for name in ("Q_FRAG", "Q_NONE"):              # 120 of 400 nt is below --min-coverage 0.5; a stranger
        assert rows[name] == [dict(zip(identify.COLUMNS, [name, "none"] + ["-"] * 8))]
    doc = json.loads(base_run["report.json"])
    assert doc["summary"] == {"queries": 8, "refs": len(refs), "unique": 5, "tied": 1, "none": 2, "device_calls": 1}
    assert [q["query"] for q in doc["queries"]] == list(U.QUERIES)
    assert [q["status"] for q in doc["queries"]] == ["unique", "unique", "unique", "tied", "unique", "unique", "none", "none"]
    assert doc["queries"][0]["hits"][0] == {"rank": 1, "ref": "REF_FLANK", "strand": "+", "identity": f["identity"], "edits": 2,
                                            "pattern": "query", "coverage": f["coverage"], "title": f["title"]}
    assert doc["queries"][7]["hits"] == []


def test_plus_strand_and_coverage_knobs(tree, tmp_path):
    root, _, _ = tree
    plus, cov = os.fspath(tmp_path / "plus"), os.fspath(tmp_path / "cov")
    assert identify.run(U.args_for(root, plus, strand="plus"), hits_fn=identify.best_hits_oracle) == 0
    rows = U.rows_of(U.outputs(plus)["report.tsv"])
    assert rows["Q_RC"][0]["status"] == "none" and rows["Q_FLANK"][0]["ref"] == "REF_FLANK"
    assert identify.run(U.args_for(root, cov, min_coverage=0.1), hits_fn=identify.best_hits_oracle) == 0
    rows = U.rows_of(U.outputs(cov)["report.tsv"])
    g = rows["Q_FRAG"][0]
    assert (g["status"], g["ref"], g["pattern"], g["edits"], g["identity"], g["coverage"]) == ("unique", "FRAG", "ref", "0", "1.0000", "0.3000")


def test_top_one_still_sees_the_tie(tree, tmp_path):
    root, _, _ = tree
    out = os.fspath(tmp_path / "top1")
    assert identify.run(U.args_for(root, out, top=1), hits_fn=identify.best_hits_oracle) == 0
    rows = U.rows_of(U.outputs(out)["report.tsv"])
    assert all(len(r) == 1 for r in rows.values()) and rows["Q_TIED"][0]["status"] == "tied" and rows["Q_SAME"][0]["status"] == "unique"


def test_wrapped_lower_case_and_gz_input_change_nothing(tree, base_run, tmp_path):
    root, _, refs = tree
    recs = identify.read_fasta(os.path.join(root, "db.fasta"))
    assert [(r.title, r.seq) for r in recs] == refs and recs[0].ref == refs[0][0].split()[0]
    for db in ("db.fasta.gz", "db_plain.fasta"):
        out = os.fspath(tmp_path / db)
        assert identify.run(U.args_for(root, out, db=db), hits_fn=identify.best_hits_oracle) == 0
        assert U.outputs(out) == base_run, db


def test_reports_do_not_depend_on_the_budget(tree, base_run, tmp_path, monkeypatch):
    root, queries, refs = tree
    for name, budget, calls in (("three", U.three_piece_budget(queries, refs), 3), ("each", 1, 2 * len(refs))):
        monkeypatch.setenv("SMX_IDENTIFY_BUDGET_BYTES", str(budget))
        out = os.fspath(tmp_path / name)
        assert identify.run(U.args_for(root, out), hits_fn=identify.best_hits_oracle) == 0
        got = U.outputs(out)
        assert got["report.tsv"] == base_run["report.tsv"], name
        doc, want = json.loads(got["report.json"]), json.loads(base_run["report.json"])
        assert doc["summary"]["device_calls"] == calls
        doc["summary"]["device_calls"] = 1
        assert doc == want, name


def test_consensus_json_as_the_query_source(tree, base_run, tmp_path):
    root, queries, _ = tree
    path = os.fspath(tmp_path / "consensus.json")
    with open(path, "w") as fh:
        json.dump({"specimens": [{"specimen": f"/run/full/pool1/sample_{name}.fastq",
                                  "clusters": [{"name": name, "consensus": seq}, {"name": name + "_x", "consensus": ""}]}
                                 for name, seq in queries]}, fh)
    out = os.fspath(tmp_path / "out")
    assert identify.run(U.args_for(root, out, consensus=path, fasta=None), hits_fn=identify.best_hits_oracle) == 0
    assert U.outputs(out) == base_run


def test_unreadable_input_is_exit_status_one(tree, tmp_path):
    root, _, _ = tree
    out = os.fspath(tmp_path / "out")
    assert identify.run(U.args_for(root, out, db="missing.fasta"), hits_fn=identify.best_hits_oracle) == 1
    assert identify.run(U.args_for(root, out, fasta=os.path.join(root, "missing.fasta")), hits_fn=identify.best_hits_oracle) == 1
    assert not os.path.exists(os.path.join(out, "report.tsv"))


def test_plan_pieces_and_keys():
    assert identify.plan_pieces([5, 5, 5, 20, 1], 10) == [(0, 2), (2, 3), (3, 4), (4, 5)]
    assert identify.plan_pieces([], 10) == [] and identify.plan_pieces([3, 3], 100) == [(0, 2)]
    key = identify.pack_key(7, 300, 12345)
    assert identify.unpack_key(key) == ((7 << 20) // 300, 7, 12345) and key < identify.NONE
    assert identify.pair_rule(100, 200, 500) == (True, True) and identify.pair_rule(100, 201, 500) == (True, False)
    assert identify.pair_rule(100, 50, 500) == (False, True) and identify.pair_rule(100, 49, 500) == (False, False)
    assert identify.pair_rule(80, 80, 1000) == (True, True)
    assert identify.revcomp(b"AACGTN") == b"NACGTT"
