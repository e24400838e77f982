"""specimux-bimera on the CPU: the rule, the parsers and the outputs, with the plain-Python twin (tests/bimera_utils.py
keys_reference) in place of the device call.  The plate (bimera_utils.Plate) has substitution-only divergence between
species, so every breakpoint is exact and the expected status of every record follows from the construction: 12 species,
4 haplotypes 1-3 edits from a species, 8 chimeras with a breakpoint at least 40 nt from each end, half of them with 1 or 2
further edits, every parent pair at least max_edits + min_gain differences apart on each side of the breakpoint.  The
tool's verdicts (from the two furthest-reaching parents) are also compared with the rule over the full matrix."""
import argparse
import gzip
import json

import pytest

import bimera_utils as U
from specimux_amd import bimera


@pytest.fixture(scope="module")
def plate():
    return U.Plate()


def args_for(tmp_path, **kw):
    base = dict(consensus=None, fasta=None, parents=None, scope="specimen", max_edits=U.MAX_EDITS, min_gain=U.MIN_GAIN,
                min_parent_ratio=2.0, report=str(tmp_path / "out.tsv"), json=str(tmp_path / "out.json"),
                clean=str(tmp_path / "clean.fasta"), debug=False)
    base.update(kw)
    return argparse.Namespace(**base)


def run_tool(tmp_path, plate, **kw):
    src = tmp_path / "consensus.json"
    src.write_text(plate.consensus_json())
    args = args_for(tmp_path, consensus=str(src), **kw)
    assert bimera.run(args, reach_fn=U.keys_reference) == 0
    rows = [dict(zip(bimera.COLUMNS, line.split("\t"))) for line in open(args.report).read().splitlines()[1:]]
    return args, {r["name"]: r for r in rows}


def test_the_plate_is_what_the_docstring_says(plate):
    kinds = [t[0] for t in plate.truth.values()]
    assert (kinds.count("species"), kinds.count("haplotype"), kinds.count("chimera")) == (12, 4, 8)
    chim = [(n, t) for n, t in plate.truth.items() if t[0] == "chimera"]
    assert sum(1 for _, t in chim if not t[4]) == 2
    by_name = {c.name: c for c in plate.called}
    edited = 0
    for name, (_, left, right, bp, _) in chim:
        seq, a, b = by_name[name].seq, by_name[left].seq, by_name[right].seq
        assert 40 <= bp <= len(seq) - 40
        edited += seq != a[:bp] + b[len(b) - (len(seq) - bp):]
    assert edited == 4


@pytest.mark.parametrize("scope", ["specimen", "plate"])
def test_every_chimera_is_found_and_nothing_else(tmp_path, plate, scope):
    args, rows = run_tool(tmp_path, plate, scope=scope)
    assert list(rows) == [c.name for c in plate.by_specimen()]
    E = U.MAX_EDITS + U.MIN_GAIN
    for name, (kind, left, right, bp, local) in plate.truth.items():
        r = rows[name]
        if kind == "chimera" and (local or scope == "plate"):
            assert r["status"] == "chimera", r
            assert (r["parent_left"], r["parent_right"]) == (left, right), r
            assert int(r["break_lo"]) <= bp <= int(r["break_hi"]), (r, bp)
            assert int(r["d2"]) == int(r["edits_left"]) + int(r["edits_right"]) <= U.MAX_EDITS
            assert r["d1"] == f">{E}" or int(r["d1"]) - int(r["d2"]) >= U.MIN_GAIN
        else:
            # the two scopes differ exactly where a parent lies in another well
            assert r["status"] in ("ok", "no-parents"), r
        if kind == "haplotype":
            assert r["status"] == "ok" and 1 <= int(r["d1"]) <= 3, r
        assert int(r["length"]) == len(next(c.seq for c in plate.called if c.name == name))
    # the major species of a well has no parent of twice its size in its well; on the plate none has
    majors = [c.name for c in plate.called if c.size == 200]
    assert all(rows[n]["status"] == "no-parents" and rows[n]["parent_left"] == "-" for n in majors)
    # --clean drops exactly the chimeras, and leaves the others as they were
    chimeras = {n for n, r in rows.items() if r["status"] == "chimera"}
    assert len(chimeras) == (6 if scope == "specimen" else 8)
    clean = open(args.clean).read()
    assert clean == "".join(f">{c.title}\n{c.seq}\n" for c in plate.by_specimen() if c.name not in chimeras)
    doc = json.load(open(args.json))
    assert doc["summary"]["chimera"] == len(chimeras) and doc["summary"]["sequences"] == 24 and doc["summary"]["device_calls"] == 1
    assert [{k: str(v) for k, v in r.items()} for r in doc["sequences"]] == list(rows.values())


@pytest.mark.parametrize("scope", ["specimen", "plate"])
def test_the_top_two_rule_is_the_full_matrix_rule(plate, scope):
    got, _ = bimera.bimera(plate.called, [], scope, U.MAX_EDITS, U.MIN_GAIN, 2.0, reach_fn=U.keys_reference)
    assert [U.verdict_tuple(v) for v in got] == U.verdicts_reference(plate.called, [], scope, U.MAX_EDITS, U.MIN_GAIN, 2.0)
    # other thresholds, other ratios: the agreement is not a property of the defaults
    for max_edits, min_gain, ratio in ((0, 1, 0.0), (3, 5, 1.0), (5, 10, 0.1)):
        got, _ = bimera.bimera(plate.called, [], scope, max_edits, min_gain, ratio, reach_fn=U.keys_reference)
        assert [U.verdict_tuple(v) for v in got] == U.verdicts_reference(plate.called, [], scope, max_edits, min_gain, ratio)


def test_a_chimera_more_abundant_than_its_parents_is_not_flagged(plate):
    called = [bimera.Called(c.name, c.specimen, 150 if plate.truth[c.name][0] == "chimera" else c.size, c.title, c.seq)
              for c in plate.called]
    got, summary = bimera.bimera(called, [], "plate", U.MAX_EDITS, U.MIN_GAIN, 2.0, reach_fn=U.keys_reference)
    assert summary["chimera"] == 0
    for c, v in zip(called, got):
        if plate.truth[c.name][0] == "chimera":
            assert v.status == "no-parents"        # 150 reads: a parent would need 300
    called = [bimera.Called(c.name, c.specimen, 60 if plate.truth[c.name][0] == "chimera" else c.size, c.title, c.seq)
              for c in plate.called]
    got, _ = bimera.bimera(called, [], "plate", U.MAX_EDITS, U.MIN_GAIN, 2.0, reach_fn=U.keys_reference)
    sizes = {c.name: c.size for c in called}
    flagged = 0
    for c, v in zip(called, got):
        kind, left, right = plate.truth[c.name][:3]
        if kind == "chimera":                      # 60 reads: only the major species (200) are parents
            both = sizes[left] >= 120 and sizes[right] >= 120
            assert v.status == ("chimera" if both else "ok") and (both or v.right is None), (c.name, U.verdict_tuple(v))
            flagged += both
    assert flagged == 1


def test_parents_from_a_pool_and_the_budget(tmp_path, plate, monkeypatch):
    """The species of another plate as --parents: a chimera whose parents are missing from the run is found through them,
    a pool record is never a query, and a budget of three pieces gives the one-piece result."""
    keep = [c for c in plate.called if plate.truth[c.name][0] != "species"]
    src = tmp_path / "called.fasta"                # wrapped lines, lower case: read as one upper-case sequence
    src.write_text("".join(f">{c.title}\n{c.seq[:60]}\n{c.seq[60:].lower()}\n" for c in keep))
    pool = tmp_path / "parents.fasta.gz"
    with gzip.open(pool, "wt") as fh:
        fh.write("".join(f">{c.name} voucher\n{c.seq}\n" for c in plate.called if plate.truth[c.name][0] == "species"))
    outs = []
    for budget in (None, sum(len(c.seq) for c in keep) + 4 * 160 + 10):
        if budget:
            monkeypatch.setenv("SMX_BIMERA_BUDGET_BYTES", str(budget))
        # a ratio of 5 keeps the run's haplotypes (40 reads) from standing in for the species they came from
        args = args_for(tmp_path, fasta=str(src), parents=str(pool), scope="specimen", min_parent_ratio=5.0)
        assert bimera.run(args, reach_fn=U.keys_reference) == 0
        outs.append((open(args.report).read(), json.load(open(args.json))))
    assert outs[0][1]["summary"]["device_calls"] == 2 and outs[1][1]["summary"]["device_calls"] == 4
    assert outs[0][0] == outs[1][0] and outs[0][1]["sequences"] == outs[1][1]["sequences"]
    rows = {r["name"]: r for r in outs[0][1]["sequences"]}
    assert list(rows) == [c.name for c in keep]
    for name, (kind, left, right, bp, _) in plate.truth.items():
        if kind == "chimera":
            assert rows[name]["status"] == "chimera" and (rows[name]["parent_left"], rows[name]["parent_right"]) == (left, right)
            assert rows[name]["break_lo"] <= bp <= rows[name]["break_hi"]
        elif kind == "haplotype":
            assert rows[name]["status"] == "ok" and rows[name]["parent_left"] != "-"


def test_inputs_that_are_refused(tmp_path, plate, caplog):
    src = tmp_path / "consensus.json"
    src.write_text(plate.consensus_json())
    with pytest.raises(ValueError, match="outside 0..15"):
        bimera.run(args_for(tmp_path, consensus=str(src), max_edits=8, min_gain=8), reach_fn=U.keys_reference)
    with pytest.raises(SystemExit) as exit_:
        bimera.main(["--consensus", str(src), "--max-edits", "8", "--min-gain", "8"])
    assert exit_.value.code == 2
    bad = tmp_path / "nosize.fasta"
    bad.write_text(">W00_c1 size=12\nACGT\n>W00_c2 share=0.5\nACGA\n")
    assert bimera.run(args_for(tmp_path, fasta=str(bad)), reach_fn=U.keys_reference) == 1
    assert "W00_c2" in caplog.text and "size=" in caplog.text
    assert bimera.run(args_for(tmp_path, consensus=str(tmp_path / "missing.json")), reach_fn=U.keys_reference) == 1
    help_text = bimera.build_parser().format_help()
    assert help_text.count("not a measured constant") == 3


def test_names_needs_and_keys():
    assert bimera.specimen_of("ONT01.01-A01_c2") == "ONT01.01-A01" and bimera.specimen_of("S_c1_h3") == "S"
    assert bimera.specimen_of("plain") == "plain"
    assert [bimera.need_of(s, 2000) for s in (0, 1, 7)] == [0, 2, 14] and bimera.need_of(3, 1500) == 5
    assert bimera.need_of(10, 1001) == 11 and bimera.need_of(10, 0) == 0
    assert bimera.unpack_key(bimera.pack_key(650, 12345)) == (650, 12345)
    assert bimera.pack_key(651, 9) < bimera.pack_key(650, 3) < bimera.pack_key(650, 4) < bimera.NONE
