"""specimux-errors on the GPU: the tool over the small plate of test_errors_cpu.py with its device calls
(clusters.adjacency, consensus.votes, errors.profile: smx_pairs.hip, smx_cons.hip, smx_profile.hip) against the same run
with the plain-Python twins, every output file byte for byte, and the planted substitutions counted exactly."""
import os

import pytest

from specimux_amd import errors
from test_errors_cpu import OUTPUTS, SUBS_PER_READ, plate, run_errors, table_rows  # noqa: F401  (plate is a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_run(plate, tmp_path_factory):  # noqa: F811
    out_dir = str(tmp_path_factory.mktemp("device"))
    argv = ["--run-dir", plate.root, "--report", os.path.join(out_dir, "errors.tsv"), "--quality", os.path.join(out_dir, "quality.tsv"),
            "--homopolymers", os.path.join(out_dir, "homopolymers.tsv"), "--reads", os.path.join(out_dir, "reads.tsv"),
            "--json", os.path.join(out_dir, "errors.json"), "--fasta", os.path.join(out_dir, "called.fasta")]
    kernel_ms = []
    assert errors.run(errors.build_parser().parse_args(argv), kernel_ms=kernel_ms) == 0
    assert kernel_ms and max(kernel_ms) > 0
    files = {}
    for name in OUTPUTS:
        with open(os.path.join(out_dir, name), "rb") as fh:
            files[name] = fh.read()
    return files


def test_device_run_equals_twin_run(plate, device_run, tmp_path):  # noqa: F811
    twin = run_errors(plate.root, str(tmp_path / "twin"))
    for name in OUTPUTS:
        assert device_run[name] == twin[name], name
    assert twin["reads.tsv"].count(b"\n") == 91 and twin["quality.tsv"].count(b"\n") == 32


def test_planted_substitutions_are_counted_exactly(device_run):
    """S_subs: 30 exact copies of a template but for SUBS_PER_READ substitutions each -- exactly that sub total, and no
    inserted or deleted base."""
    reads = [r for r in table_rows(device_run["reads.tsv"], errors.READ_COLUMNS) if r.name == "S_subs_c1"]
    assert len(reads) == 30 and all(int(r.sub) == SUBS_PER_READ and int(r.match) == 300 - SUBS_PER_READ for r in reads)
    assert sum(int(r.ins_bases) + int(r.ins_events) + int(getattr(r, "del")) + int(r.other) for r in reads) == 0
    row = next(r for r in table_rows(device_run["errors.tsv"], errors.COLUMNS) if r.specimen.endswith("S_subs.fastq"))
    assert row.sub_per_kb == f"{1000 * SUBS_PER_READ / 300:.3f}" and row.ins_per_kb == row.del_per_kb == "0.000"
