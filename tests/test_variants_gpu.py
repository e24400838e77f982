"""specimux-variants on the GPU: the two scenarios of test_variants_cpu.py with the device calls (clusters.adjacency,
consensus.votes, variants.phase) against the same run over their plain-Python twins: FASTA, report, sites and JSON byte
for byte."""
import os
import subprocess
import sys

import pytest

from cons_utils import votes_reference
from specimux_amd import clusters, consensus, variants
from test_variants_cpu import OUTPUTS, check_two_haplotypes, one_template, run_variants, two_haplotypes, write_specimen
from variants_utils import phase_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """A specimen of two haplotypes and one of a single template with a homopolymer error, in one tree."""
    root = str(tmp_path_factory.mktemp("variants") / "out")
    rng, templates, reads = two_haplotypes(1)
    write_specimen(root, "S_two", rng, reads)
    rng, _full, reads = one_template(1)
    write_specimen(root, "S_one", rng, reads)
    return root, templates


@pytest.fixture(scope="module")
def twin_files(tree, tmp_path_factory):
    return run_variants(tree[0], str(tmp_path_factory.mktemp("twin")), clusters.adjacency_oracle, votes_reference, phase_reference)


def test_tree_files_equal_the_twin_run(tree, twin_files, tmp_path):
    files = run_variants(tree[0], str(tmp_path / "gpu"), clusters.adjacency, consensus.votes, variants.phase)
    assert sorted(files) == sorted(OUTPUTS)
    for name in files:
        assert files[name] == twin_files[name], name
    names = [ln[1:].split()[0] for ln in files["variants.fasta"].decode().splitlines() if ln.startswith(">")]
    assert names == ["S_one_c1", "S_two_c1_h1", "S_two_c1_h2"]


def test_each_specimen_alone(tree, tmp_path):
    root, templates = tree
    two = os.path.join(root, "full", "POOL", "S_two.fastq")
    files = run_variants(root, str(tmp_path / "two"), clusters.adjacency, consensus.votes, variants.phase, fastq=two)
    check_two_haplotypes(files, templates, name="S_two")
    twin = run_variants(root, str(tmp_path / "two_twin"), clusters.adjacency_oracle, votes_reference, phase_reference, fastq=two)
    assert files == twin
    one = os.path.join(root, "full", "POOL", "S_one.fastq")
    files = run_variants(root, str(tmp_path / "one"), clusters.adjacency, consensus.votes, variants.phase, fastq=one)
    twin = run_variants(root, str(tmp_path / "one_twin"), clusters.adjacency_oracle, votes_reference, phase_reference, fastq=one)
    assert files == twin and b"_h1" not in files["variants.fasta"]


def test_module_runs_as_a_command(tree, twin_files, tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "specimux_amd.variants", "--run-dir", tree[0], "--fasta",
                          str(tmp_path / "v.fasta"), "--sites", str(tmp_path / "s.tsv")], cwd=repo, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "Split 1 of 2 cluster(s) of 2 specimen(s) into 2 haplotype(s) in 1 phase call(s)" in out.stderr
    assert (tmp_path / "v.fasta").read_bytes() == twin_files["variants.fasta"]
    assert (tmp_path / "s.tsv").read_bytes() == twin_files["sites.tsv"]
