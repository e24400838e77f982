"""specimux-consensus on the GPU: the tool over a synthetic tree with the device calls against the same run over their
plain-Python twins, byte for byte, under one and under several device calls, and the recovery of a known template."""
import json
import random

import pytest

from clusters_utils import mutate, rand_seq, run_tool, write_tree
from cons_utils import consensus_reference, votes_reference
from specimux_amd import clusters, consensus
from test_consensus_cpu import check_outputs, run_consensus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("consensus") / "out")
    write_tree(random.Random(71), root)
    return root


@pytest.fixture(scope="module")
def twin_files(tree, tmp_path_factory):
    return run_consensus(tree, str(tmp_path_factory.mktemp("twin")), clusters.adjacency_oracle, votes_reference)


def test_tree_files_equal_the_twin_run(tree, twin_files, tmp_path):
    files = run_consensus(tree, str(tmp_path / "gpu"), clusters.adjacency, consensus.votes)
    check_outputs(files, run_tool(tree, str(tmp_path / "cl"), clusters.adjacency))
    assert sorted(files) == sorted(twin_files)
    for name in files:
        assert files[name] == twin_files[name], name


def test_several_device_calls_give_the_same_files(tree, twin_files, tmp_path, monkeypatch):
    monkeypatch.setenv("SMX_CLUSTERS_BUDGET_BYTES", "30000")   # less than two specimen files: a call per specimen
    ms = []
    argv = ["--run-dir", tree, "--fasta", str(tmp_path / "c.fasta"), "--report", str(tmp_path / "r.tsv"),
            "--json", str(tmp_path / "r.json")]
    assert consensus.run(consensus.build_parser().parse_args(argv), kernel_ms=ms) == 0
    doc = json.loads((tmp_path / "r.json").read_text())
    twin = json.loads(twin_files["report.json"])
    assert doc["summary"]["vote_calls"] == len(ms) > twin["summary"]["vote_calls"] and all(x > 0 for x in ms)
    assert doc["specimens"] == twin["specimens"]
    assert (tmp_path / "c.fasta").read_bytes() == twin_files["consensus.fasta"]
    assert (tmp_path / "r.tsv").read_bytes() == twin_files["report.tsv"]


@pytest.mark.parametrize("rate", [0.05, 0.10])
def test_truth_is_recovered_through_the_device(rate):
    for seed in (1, 2, 3):
        rng = random.Random(seed)
        truth = rand_seq(rng, 300)
        reads = [mutate(rng, truth, rate) for _ in range(30)]
        assert consensus_reference(reads[0], reads[1:], rounds=4, votes_fn=consensus.votes) == truth, seed


def test_hard_inputs_equal_the_twin():
    """Homopolymer-rich templates and few voters: the template need not come back; the device and the twin agree."""
    for seed in (1, 2, 3, 4):
        rng = random.Random(100 + seed)
        truth = "".join(rng.choice("ACGT") * rng.randrange(1, 9) for _ in range(60))
        reads = [mutate(rng, truth, 0.08) for _ in range(12 if seed % 2 else 30)]
        got = consensus_reference(reads[0], reads[1:], rounds=4, votes_fn=consensus.votes)
        assert got == consensus_reference(reads[0], reads[1:], rounds=4), seed


def test_module_runs_as_a_command(tree, twin_files, tmp_path):
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "specimux_amd.consensus", "--run-dir", tree, "--fasta",
                          str(tmp_path / "c.fasta")], cwd=repo, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "Polished 3 cluster(s) of 3 specimen(s) (1 mixed)" in out.stderr
    assert (tmp_path / "c.fasta").read_bytes() == twin_files["consensus.fasta"]
