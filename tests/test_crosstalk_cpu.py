"""specimux-crosstalk on the CPU: the tool run over the synthetic run of tests/crosstalk_utils.py with the oracle in
place of the device call (crosstalk.nearest_oracle) recovers the planted outcome exactly; the class rule, the flag rule
and the --refs name mapping at their boundaries.  No GPU needed."""
import json
import os

import pytest

from specimux_amd import crosstalk

import crosstalk_utils as U


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    root = tmp_path_factory.mktemp("crosstalk_run")
    paths = U.build_run(os.fspath(root))
    out = os.fspath(root / "out")
    assert crosstalk.run(U.args_for(root, out), nearest_fn=crosstalk.nearest_oracle) == 0
    with open(os.path.join(out, "report.json")) as fh:
        doc = json.load(fh)
    return root, paths, out, doc


def by_name(doc, paths):
    spec = {s["specimen"]: s for s in doc["specimens"]}
    return {name: spec[p] for name, p in paths.items()}


def test_the_planted_outcome_is_recovered(planted):
    root, paths, out, doc = planted
    s = by_name(doc, paths)
    assert {n: x["status"] for n, x in s.items()} == {"SPEC_A": "contaminated", "SPEC_B": "clean", "SPEC_C": "clean",
                                                      "SPEC_D": "clean", "SPEC_E": "no_reference", "SPEC_F": "clean"}
    (a,) = s["SPEC_A"]["sources"]
    assert (a["source"], a["source_ref"], a["reads"]) == (paths["SPEC_B"], "SPEC_B_c1", 6) and a["share"] == round(6 / 26, 4)
    assert a["ref_distance"] is not None and a["ref_distance"] > 100 and a["min_distance"] <= a["median_distance"] <= 30
    (e,) = s["SPEC_E"]["sources"]
    assert (e["source"], e["reads"], e["ref_distance"]) == (paths["SPEC_B"], 5, None)
    assert (s["SPEC_E"]["foreign"], s["SPEC_E"]["reads"], s["SPEC_E"]["refs"]) == (5, 5, 0)
    assert (s["SPEC_A"]["own"], s["SPEC_A"]["foreign"]) == (20, 6)
    assert (s["SPEC_B"]["own"], s["SPEC_B"]["reads"]) == (20, 20)
    # C holds three reads of D's template: nearer to D's ref, but the refs are 3 < 5 edits apart
    assert (s["SPEC_C"]["own"], s["SPEC_C"]["ambiguous"], s["SPEC_C"]["foreign"], s["SPEC_C"]["sources"]) == (20, 3, 0, [])
    assert (s["SPEC_D"]["own"] + s["SPEC_D"]["ambiguous"], s["SPEC_D"]["foreign"], s["SPEC_D"]["sources"]) == (20, 0, [])
    assert (s["SPEC_F"]["own"], s["SPEC_F"]["unplaced"], s["SPEC_F"]["foreign"]) == (20, 4, 0)
    sm = doc["summary"]
    assert (sm["specimens"], sm["read"], sm["failed"], sm["refs"], sm["reads"], sm["device_calls"]) == (6, 6, 0, 6, 118, 1)
    assert (sm["placed"], sm["foreign"], sm["foreign_share"]) == (114, 11, round(11 / 114, 4))
    assert (sm["flagged_sources"], sm["contaminated"]) == (2, 1)


def test_the_report_and_the_read_table(planted):
    root, paths, out, doc = planted
    rows = [line.split("\t") for line in open(os.path.join(out, "report.tsv")).read().split("\n")]
    assert tuple(rows[0]) == crosstalk.COLUMNS and rows[7] == [""] and tuple(rows[8]) == crosstalk.SOURCE_COLUMNS
    assert rows[1] == [paths["SPEC_A"], "contaminated", "26", "20", "0", "0", "6", "1"]
    assert rows[5] == [paths["SPEC_E"], "no_reference", "5", "0", "0", "0", "5", "0"]
    assert rows[9][:4] == [paths["SPEC_A"], paths["SPEC_B"], "SPEC_B_c1", "6"] and rows[9][4] == f"{6 / 26:.4f}"
    assert rows[10][:4] == [paths["SPEC_E"], paths["SPEC_B"], "SPEC_B_c1", "5"] and rows[10][7] == "-"
    assert len(rows) == 12 and rows[11] == [""]
    reads = [line.split("\t") for line in open(os.path.join(out, "reads.tsv")).read().splitlines()]
    assert tuple(reads[0]) == crosstalk.READ_COLUMNS and len(reads) == 1 + 118
    e = [r for r in reads if r[0] == paths["SPEC_E"]]
    assert len(e) == 5 and all(r[2:5] == ["foreign", "-", "-"] and r[5] == "SPEC_B_c1" and 0 <= int(r[6]) <= 30 for r in e)
    junk = [r for r in reads if r[2] == "unplaced"]
    assert len(junk) == 4 and all(r[0] == paths["SPEC_F"] and r[3:] == ["-", "-", "-", "-"] for r in junk)
    assert all(r[1].startswith("SPEC_") and " " not in r[1] for r in reads[1:])


def test_the_knobs_at_their_boundaries(planted, tmp_path):
    root, paths, out, doc = planted

    def rerun(name, **kw):
        o = os.fspath(tmp_path / name)
        assert crosstalk.run(U.args_for(root, o, **kw), nearest_fn=crosstalk.nearest_oracle) == 0
        with open(os.path.join(o, "report.json")) as fh:
            return by_name(json.load(fh), paths)
    s = rerun("r6", min_reads=6)                   # --min-reads equal to the count: flagged
    assert s["SPEC_A"]["status"] == "contaminated" and s["SPEC_E"]["sources"] == [] and s["SPEC_E"]["status"] == "no_reference"
    s = rerun("r7", min_reads=7)
    assert s["SPEC_A"]["status"] == "clean" and s["SPEC_A"]["foreign"] == 6
    s = rerun("s3", min_separation=3)              # the refs of C and D are exactly 3 apart: D == --min-separation is foreign
    assert (s["SPEC_C"]["ambiguous"], s["SPEC_C"]["foreign"], s["SPEC_C"]["status"]) == (0, 3, "clean")
    s = rerun("s3r3", min_separation=3, min_reads=3)
    assert s["SPEC_C"]["status"] == "contaminated" and s["SPEC_C"]["sources"][0]["ref_distance"] == 3
    s = rerun("s4", min_separation=4)
    assert (s["SPEC_C"]["ambiguous"], s["SPEC_C"]["foreign"]) == (3, 0)


def test_the_class_rule():
    asked = []

    def dist(d):
        def f(a, b):
            asked.append((a, b))
            return d
        return f
    c = crosstalk.classify
    assert c(None, None, dist(0), 5) == "unplaced"
    assert c((7, 1), None, dist(0), 5) == "own"
    assert c((7, 1), (7, 0), dist(99), 5) == "own"             # a tie is own, whatever the refs
    assert c((7, 1), (8, 0), dist(99), 5) == "own"
    assert c(None, (30, 2), dist(0), 5) == "foreign"
    assert asked == []                                          # the ref distance is not needed so far
    assert c((7, 1), (6, 0), dist(5), 5) == "foreign"           # D equal to --min-separation
    assert c((7, 1), (6, 0), dist(4), 5) == "ambiguous"
    assert asked == [(1, 0), (1, 0)]
    assert crosstalk.decode(2**64 - 1) is None and crosstalk.decode((9 << 32) | 4) == (9, 4)
    refs = [crosstalk.Ref("a", "a", 0, "ACGTACGT"), crosstalk.Ref("b", "b", 1, "ACGAACG")]
    rd = crosstalk.RefDistances(refs)
    assert rd(0, 1) == 2 and rd(1, 0) == 2 and rd(1, 1) == 0 and list(rd.cache) == [(0, 1), (1, 1)]


def test_ref_names_map_to_specimens(planted, tmp_path):
    root, paths, out, doc = planted
    assert crosstalk.ref_specimen_name("SPEC_A_c1 size=20") == "SPEC_A"
    assert crosstalk.ref_specimen_name("SPEC_A_c12") == "SPEC_A" and crosstalk.ref_specimen_name("SPEC_A") == "SPEC_A"
    assert crosstalk.ref_specimen_name("SPEC_c1_x") == "SPEC_c1_x" and crosstalk.ref_specimen_name("S_c") == "S_c"
    files = sorted(paths.values())
    refs = crosstalk.refs_from_fasta(os.path.join(root, "refs.fasta"), files)
    assert [r.name for r in refs] == ["SPEC_A_c1", "SPEC_B_c1", "SPEC_C_c1", "SPEC_D_c1", "SPEC_F_c1", "GHOST_c1"]
    assert [r.file for r in refs] == [0, 1, 2, 3, 5, None] and all(len(r.seq) == 300 for r in refs)
    assert crosstalk.ref_groups(refs, 6) == [0, 1, 2, 3, 5, 6]     # a ref that matches no file: a group of its own
    # --consensus carries the files: the same refs, the same report
    o = os.fspath(tmp_path / "cons")
    args = U.args_for(root, o, refs=None, consensus=os.path.join(root, "consensus.json"))
    assert crosstalk.run(args, nearest_fn=crosstalk.nearest_oracle) == 0
    assert U.outputs(o) == U.outputs(out)
    # a second pool with a specimen of the same name: --refs cannot tell them apart and says so; --consensus can
    two = os.fspath(tmp_path / "two_pools")
    U.build_run(two)
    other = os.path.join(two, "full", "pool2")
    os.makedirs(other)
    with open(os.path.join(other, "SPEC_B.fastq"), "w") as fh:
        fh.write("@x\nACGT\n+\nIIII\n")
    with pytest.raises(ValueError) as err:
        crosstalk.run(U.args_for(two, os.path.join(two, "out")), nearest_fn=crosstalk.nearest_oracle)
    assert os.path.join("pool1", "SPEC_B.fastq") in str(err.value) and os.path.join("pool2", "SPEC_B.fastq") in str(err.value)
    args = U.args_for(two, os.path.join(two, "out"), refs=None, consensus=os.path.join(two, "consensus.json"))
    assert crosstalk.run(args, nearest_fn=crosstalk.nearest_oracle) == 0
    with open(os.path.join(two, "out", "report.json")) as fh:
        spec = {s["specimen"]: s for s in json.load(fh)["specimens"]}
    assert spec[os.path.join(other, "SPEC_B.fastq")]["status"] == "no_reference"
    assert spec[os.path.join(two, "full", "pool1", "SPEC_B.fastq")]["status"] == "clean"


def test_no_readable_file_is_status_1(tmp_path):
    os.makedirs(tmp_path / "full" / "pool1")
    with open(tmp_path / "full" / "pool1" / "S.fastq", "w") as fh:
        fh.write("not a fastq\n")
    with open(tmp_path / "refs.fasta", "w") as fh:
        fh.write(">S_c1\nACGT\n")
    assert crosstalk.run(U.args_for(tmp_path, os.fspath(tmp_path / "out")), nearest_fn=crosstalk.nearest_oracle) == 1
