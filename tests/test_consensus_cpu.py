"""specimux-consensus without a GPU: the call rule on hand-built vote tables, the tool over a synthetic tree with the
plain-Python twins of its two device calls (clusters.adjacency_oracle, cons_utils.votes_reference), and the recovery of
a known template from its noisy reads."""
import json
import os
import random
import types

import numpy as np
import pytest

from clusters_utils import mutate, rand_seq, report_rows, run_tool, write_tree
from cons_utils import NO_ROW, consensus_reference, reduce_rows, row_reference, votes_reference
from specimux_amd import clusters, consensus


def table_of(draft, reads, k=-1):
    """The vote table of `reads` over `draft` and the number that voted."""
    rows = [row for d, row in (row_reference(draft.encode(), r.encode(), k) for r in reads) if d >= 0]
    return reduce_rows(np.array(rows, dtype=np.uint32).reshape(len(rows), len(draft) + 1), len(draft)), len(rows)


def blank(m):
    return np.zeros((m + 1, 26), dtype=np.uint32)


def test_row_reference_format():
    # draft ACGT, read TTACTT: TT before position 0, T for G
    d, row = row_reference(b"ACGT", b"TTACTT", -1)
    assert d == 3 and row == [0 | 2 << 3 | 3 << 11 | 3 << 14, 1, 3, 3, 7]
    d, row = row_reference(b"AAAA", b"AAA", -1)                 # the walk takes the diagonal while it can: the gap is first
    assert d == 1 and row == [5, 0, 0, 0, 7]
    d, row = row_reference(b"AAA", b"AAAA", -1)
    assert d == 1 and row == [0 | 1 << 3, 0, 0, 7]
    d, row = row_reference(b"ACGT", b"ACNT", 0)
    assert d == -1 and row == [NO_ROW] * 5
    d, row = row_reference(b"ACGT", b"ACNT", 1)
    assert d == 1 and row == [0, 1, 4, 3, 7]
    d, row = row_reference(b"AC", b"ACGGGGGG", -1)              # six inserted, four slots
    assert d == 6 and row == [0, 1, 7 | 6 << 3 | 2 << 11 | 2 << 14 | 2 << 17 | 2 << 20]
    d, row = row_reference(b"ACG", b"", 3)
    assert d == 3 and row == [5, 5, 5, 7]


def test_call_rule_ties():
    t = blank(3)
    t[0, [1, 2]] = 3                                            # C and G tie, the draft has G: the draft's base
    t[1, [2, 3]] = 3                                            # G and T tie, the draft has A: the lowest code
    t[2, 4] = 6                                                 # no ACGT vote at all: the draft's base
    assert consensus.call_consensus("GAN", t, 6) == "GGN"
    t[0, 0] = 4                                                 # a plain majority beats the draft
    assert consensus.call_consensus("GAN", t, 10) == "AGN"


def test_call_rule_half_deletions_keep_the_base():
    t = blank(2)
    t[0, 5], t[0, 1] = 5, 5
    t[1, 5], t[1, 1] = 6, 4
    assert consensus.call_consensus("CC", t, 10) == "C"         # 5 of 10: exactly half, kept; 6 of 10: dropped
    assert consensus.call_consensus("CC", t, 11) == "C"
    assert consensus.call_consensus("CC", t, 12) == "CC"        # 6 of 12: exactly half, kept
    assert consensus.call_consensus("CC", t, 9) == ""           # 5 of 9 and 6 of 9: both dropped


def test_call_rule_insertion_slots_stop_at_the_first_minority():
    t = blank(1)
    t[0, 0] = 10
    t[0, 6 + 2], t[0, 6 + 3] = 3, 2                             # slot 0: 5 of 10 reads have an insertion: exactly half
    assert consensus.call_consensus("A", t, 10) == "A"
    t[0, 6 + 2], t[0, 6 + 3] = 3, 3
    t[0, 6 + 4] = 1                                             # 7 of 10 vote in slot 0: emitted; G and T tie: the lowest
    t[0, 11 + 1] = 5                                            # slot 1: exactly half: stops
    t[0, 16 + 0] = 9                                            # slot 2 has a majority but is never reached
    assert consensus.call_consensus("A", t, 10) == "GA"
    t[0, 11 + 1] = 6
    assert consensus.call_consensus("A", t, 10) == "GCAA"
    t[1, 6 + 3] = 6                                             # after the last base
    assert consensus.call_consensus("A", t, 10) == "GCAAT"


def test_votes_reference_counts_slots():
    table, n = table_of("ACGT", ["ACGT", "AGGGCGT", "ACG", "TTTTTTTT"], k=3)
    assert n == 3                                               # the last read is above the limit
    assert table[0, :6].tolist() == [3, 0, 0, 0, 0, 0] and table[3, :6].tolist() == [0, 0, 0, 2, 0, 1]
    assert table[1, 6:].tolist() == [0, 0, 1, 0, 0] + [0, 0, 1, 0, 0] + [0, 0, 1, 0, 0] + [0] * 5
    assert not table[4].any()


@pytest.mark.parametrize("rate", [0.05, 0.10])
def test_truth_is_recovered(rate):
    """30 reads of a 300-nt template: the first is the draft, the other 29 vote.  A condition, not a tolerance."""
    for seed in range(1, 7):
        rng = random.Random(seed)
        truth = rand_seq(rng, 300)
        reads = [mutate(rng, truth, rate) for _ in range(30)]
        assert consensus_reference(reads[0], reads[1:], rounds=4) == truth, seed


# ------------------------------------------------------------------------------------------------ the tool
def run_consensus(root, out_dir, adjacency_fn, votes_fn, fastq=None, **options):
    """consensus.run on the tree (or one file) with every output switched on; returns {output name: bytes}."""
    os.makedirs(out_dir, exist_ok=True)
    argv = ["--fastq", fastq] if fastq else ["--run-dir", root]
    argv += ["--fasta", os.path.join(out_dir, "consensus.fasta"), "--report", os.path.join(out_dir, "report.tsv"),
             "--json", os.path.join(out_dir, "report.json")]
    for key, val in options.items():
        argv += ["--" + key.replace("_", "-"), str(val)]
    assert consensus.run(consensus.build_parser().parse_args(argv), adjacency_fn=adjacency_fn, votes_fn=votes_fn) == 0
    files = {}
    for name in ("consensus.fasta", "report.tsv", "report.json"):
        with open(os.path.join(out_dir, name), "rb") as fh:
            files[name] = fh.read()
    return files


def fasta_records(data):
    lines = data.decode("latin-1").splitlines()
    assert len(lines) % 2 == 0 and all(ln.startswith(">") for ln in lines[0::2])
    out = []
    for head, seq in zip(lines[0::2], lines[1::2]):
        name, *fields = head[1:].split()
        out.append(types.SimpleNamespace(name=name, seq=seq, **dict(f.split("=") for f in fields)))
    return out


def check_outputs(files, cluster_files):
    """One record for S_one, two for S_two, none for S_six; the three outputs agree with each other and with clusters'."""
    recs = fasta_records(files["consensus.fasta"])
    assert [r.name for r in recs] == ["S_one_c1", "S_two_c1", "S_two_c2"]
    assert [r.size for r in recs] == ["40", "28", "12"] and [r.share for r in recs] == ["1.0000", "0.7000", "0.3000"]
    lines = files["report.tsv"].decode("latin-1").splitlines()
    assert lines[0].split("\t") == list(consensus.COLUMNS)
    rows = [types.SimpleNamespace(**dict(zip(consensus.COLUMNS, ln.split("\t")))) for ln in lines[1:]]
    doc = json.loads(files["report.json"])
    docs = [(s, c) for s in doc["specimens"] for c in s["clusters"]]
    assert len(rows) == len(recs) == len(docs) == doc["summary"]["polished"] == 3
    assert [s["specimen"].endswith("S_six.fastq") and not s["clusters"] for s in doc["specimens"]] == [False, True, False]
    cl_rows = {(r.specimen, r.cluster): r for r in report_rows(cluster_files["report.tsv"])}
    for rec, row, (spec, c) in zip(recs, rows, docs):
        assert rec.name == row.name == c["name"] and rec.seq == c["consensus"]
        assert (rec.size, rec.aligned, rec.rounds, rec.edits) == (row.size, row.aligned, row.rounds, row.edits) \
            == tuple(str(c[x]) for x in ("size", "aligned", "rounds", "edits"))
        assert rec.share == row.share == f"{c['share']:.4f}" and int(row.length) == len(rec.seq) == c["length"]
        assert row.stop == c["stop"] and row.stop in ("converged", "rounds")
        assert row.specimen == spec["specimen"] and row.status == spec["status"]
        cl = cl_rows[(row.specimen, row.cluster)]                # clusters' own report of the same run
        assert (cl.size, cl.share, cl.status, cl.sampled) == (row.size, row.share, row.status, row.sampled)
        assert 1 <= int(rec.rounds) <= 3 and int(rec.size) - 2 <= int(rec.aligned) <= int(rec.size)
    assert [r.status for r in rows] == ["ok", "mixed", "mixed"]
    return recs


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("consensus") / "out")
    write_tree(random.Random(51), root)
    return root


def test_outputs_of_a_synthetic_tree(tree, tmp_path):
    files = run_consensus(tree, str(tmp_path / "res"), clusters.adjacency_oracle, votes_reference)
    recs = check_outputs(files, run_tool(tree, str(tmp_path / "cl"), clusters.adjacency_oracle))
    # the consensus of a cluster is closer to every one of its reads' template than a read is: at 2 % error the centre
    # of 40 reads differs from its consensus by a few edits at most, and polishing again changes nothing
    centres = {r.name: r for r in fasta_records(run_tool(tree, str(tmp_path / "cl2"), clusters.adjacency_oracle)["centres.fasta"])}
    for r in recs:
        assert int(r.edits) == consensus.nw_distance(centres[r.name].seq, r.seq) <= 15
    again = consensus_reference(recs[0].seq, [x.seq for x in clusters.read_records(os.path.join(tree, "full", "POOL", "S_one.fastq"))])
    assert again == recs[0].seq


def test_rounds_and_low_aligned(tree, tmp_path):
    one = run_consensus(tree, str(tmp_path / "r1"), clusters.adjacency_oracle, votes_reference, rounds=1)
    rows = json.loads(one["report.json"])
    assert [c["rounds"] for s in rows["specimens"] for c in s["clusters"]] == [1, 1, 1] and rows["summary"]["vote_calls"] == 1
    assert {c["stop"] for s in rows["specimens"] for c in s["clusters"]} <= {"rounds", "converged"}

    def few(reads, ks, jobs, kernel_ms=None):                    # a device on which only four reads ever align
        tables, aligned = votes_reference(reads, ks, jobs, kernel_ms)
        return tables, [min(a, 4) for a in aligned]
    low = json.loads(run_consensus(tree, str(tmp_path / "low"), clusters.adjacency_oracle, few)["report.json"])
    centres = fasta_records(run_tool(tree, str(tmp_path / "cl"), clusters.adjacency_oracle)["centres.fasta"])
    got = [c for s in low["specimens"] for c in s["clusters"]]
    assert [(c["stop"], c["aligned"], c["rounds"], c["edits"]) for c in got] == [("low_aligned", 4, 1, 0)] * 3
    assert [c["consensus"] for c in got] == [r.seq for r in centres]   # the last draft is kept: the centre


def test_an_empty_call_keeps_the_previous_draft():
    def all_deleted(reads, ks, jobs, kernel_ms=None):
        tables = []
        for d, _, n in jobs:
            t = blank(len(reads[d]))
            t[:-1, 5] = n
            tables.append(t)
        return tables, [n for _, _, n in jobs]
    done, calls = consensus.polish([["ACGT"] * 6], 0.9, 3, 5, all_deleted)
    assert done == [("ACGT", 6, 1, "empty")] and calls == 1


def test_single_file_and_budget(tree, tmp_path, monkeypatch):
    whole = run_consensus(tree, str(tmp_path / "all"), clusters.adjacency_oracle, votes_reference)
    fastq = os.path.join(tree, "full", "POOL", "S_two.fastq")
    one = run_consensus(tree, str(tmp_path / "one"), clusters.adjacency_oracle, votes_reference, fastq=fastq)
    assert fasta_records(one["consensus.fasta"])[0].seq == fasta_records(whole["consensus.fasta"])[1].seq
    assert one["report.tsv"].splitlines()[1:] == whole["report.tsv"].splitlines()[2:]
    # a budget of one specimen per call: the same sequences from more vote calls
    monkeypatch.setenv("SMX_CLUSTERS_BUDGET_BYTES", "30000")
    calls = []

    def counting(reads, ks, jobs, kernel_ms=None):
        calls.append(len(jobs))
        return votes_reference(reads, ks, jobs, kernel_ms)
    split = run_consensus(tree, str(tmp_path / "split"), clusters.adjacency_oracle, counting)
    assert split["consensus.fasta"] == whole["consensus.fasta"] and split["report.tsv"] == whole["report.tsv"]
    assert set(calls) == {1, 2} and json.loads(split["report.json"])["summary"]["vote_calls"] == len(calls)
