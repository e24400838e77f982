"""specimux-clusters on the GPU: a tree of three specimens with known clusters through the tool, its output files byte for
byte against the run over the oracle twin of the device call, the sampling, and the single-file mode."""
import os
import random

import numpy as np
import pytest

from clusters_utils import report_rows, run_tool, write_tree
from specimux_amd import clusters

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("clusters") / "out")
    labels = write_tree(random.Random(41), root)
    return root, labels


@pytest.fixture(scope="module")
def oracle_files(tree, tmp_path_factory):
    return run_tool(tree[0], str(tmp_path_factory.mktemp("oracle")), clusters.adjacency_oracle)


def test_tree_clusters_and_files_equal_the_oracle_run(tree, oracle_files, tmp_path):
    root, labels = tree
    files = run_tool(root, str(tmp_path / "gpu"), clusters.adjacency)
    by = {}
    for r in report_rows(files["report.tsv"]):
        by.setdefault(os.path.basename(r.specimen), []).append(r)
    assert [(r.size, r.status) for r in by["S_one.fastq"]] == [("40", "ok")]
    assert [(r.size, r.status) for r in by["S_two.fastq"]] == [("28", "mixed"), ("12", "mixed")]
    assert [(r.size, r.status) for r in by["S_six.fastq"]] == [("1", "ok")] * 6
    # the two templates come apart exactly
    recs = clusters.read_records(os.path.join(root, "full", "POOL", "S_two.fastq"))
    for rank, label in ((1, 0), (2, 1)):
        want = b"".join(r.raw for r, x in zip(recs, labels["S_two"]) if x == label)
        assert files[os.path.join("split", "POOL", f"S_two.c{rank}.fastq")] == want
    assert sorted(files) == sorted(oracle_files)
    for name in files:
        assert files[name] == oracle_files[name], name


def test_adjacency_equals_the_oracle_twin(tree):
    root, _ = tree
    specimens = []
    for name in ("S_one", "S_two", "S_six"):
        recs = clusters.read_records(os.path.join(root, "full", "POOL", name + ".fastq"))
        specimens.append(([r.seq.encode("latin-1") for r in recs], [int(len(r.seq) * (1 - 0.9)) for r in recs]))
    specimens.append(([], []))
    specimens.append(([b"ACGT"], [0]))
    ms = []
    got = clusters.adjacency(specimens, ms)
    want = clusters.adjacency_oracle(specimens)
    assert len(ms) == 1 and ms[0] > 0
    assert [g.shape for g in got] == [(40, 40), (40, 40), (6, 6), (0, 0), (1, 1)]
    for g, w in zip(got, want):
        assert g.dtype == bool and np.array_equal(g, w)


def test_max_reads_samples_the_best_by_quality(tree, tmp_path):
    root, _ = tree
    files = run_tool(root, str(tmp_path / "gpu"), clusters.adjacency, max_reads=20)
    again = run_tool(root, str(tmp_path / "oracle"), clusters.adjacency_oracle, max_reads=20)
    assert files == again
    rows = report_rows(files["report.tsv"])
    assert {(os.path.basename(r.specimen), r.reads, r.sampled) for r in rows} == {
        ("S_one.fastq", "40", "20"), ("S_two.fastq", "40", "20"), ("S_six.fastq", "6", "6")}
    for name in ("S_one", "S_two"):
        recs = clusters.read_records(os.path.join(root, "full", "POOL", name + ".fastq"))
        order = sorted(range(40), key=lambda i: clusters.mean_quality(recs[i].qual), reverse=True)   # stable
        keep = {recs[i].id for i in order[:20]}
        got = set()
        for f, data in files.items():
            if os.path.basename(f).startswith(name + ".c"):
                (tmp_path / "x.fastq").write_bytes(data)
                got |= {r.id for r in clusters.read_records(str(tmp_path / "x.fastq"))}
        sizes = [int(r.size) for r in rows if os.path.basename(r.specimen) == name + ".fastq"]
        assert sum(sizes) == 20 and got <= keep
        assert len(got) == sum(s for s in sizes if s >= 5)


def test_single_file_equals_its_rows_of_the_run(tree, oracle_files, tmp_path):
    root, _ = tree
    fastq = os.path.join(root, "full", "POOL", "S_two.fastq")
    files = run_tool(root, str(tmp_path / "one"), clusters.adjacency, fastq=fastq)
    lines = files["report.tsv"].decode().splitlines()
    want = [ln for ln in oracle_files["report.tsv"].decode().splitlines() if ln.split("\t")[0] == fastq]
    assert lines[1:] == want and len(want) == 2
    assert files[os.path.join("split", "POOL", "S_two.c2.fastq")] == oracle_files[os.path.join("split", "POOL", "S_two.c2.fastq")]


def test_module_runs_as_a_command(tree, tmp_path):
    import subprocess
    import sys
    root, _ = tree
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "specimux_amd.clusters", "--run-dir", root, "--report",
                          str(tmp_path / "r.tsv")], cwd=repo, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "Clustered 3 of 3 specimen(s): 1 mixed; 1575 read pairs compared" in out.stderr
    assert len((tmp_path / "r.tsv").read_text().splitlines()) == 1 + 1 + 2 + 6
