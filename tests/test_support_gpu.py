"""specimux-support on the GPU: the tool over the small plate of test_support_cpu.py with its device calls
(clusters.adjacency, consensus.votes, support.resample: smx_pairs.hip, smx_cons.hip, smx_resample.hip) against the same
run with the plain-Python twins, every output file byte for byte."""
import os

import pytest

from specimux_amd import support
from test_support_cpu import OUTPUTS, SEED, plate, run_support  # noqa: F401  (plate is a fixture)

pytestmark = pytest.mark.gpu


def test_device_run_equals_twin_run(plate, tmp_path):  # noqa: F811
    twin = run_support(plate.root, str(tmp_path / "twin"), depths="3,5,10,20", seed=SEED)
    out_dir = str(tmp_path / "device")
    os.makedirs(out_dir)
    argv = ["--run-dir", plate.root, "--depths", "3,5,10,20", "--seed", str(SEED),
            "--report", os.path.join(out_dir, "support.tsv"), "--json", os.path.join(out_dir, "support.json"),
            "--columns", os.path.join(out_dir, "columns.tsv"), "--masked", os.path.join(out_dir, "masked.fasta"),
            "--fasta", os.path.join(out_dir, "called.fasta")]
    kernel_ms = []
    assert support.run(support.build_parser().parse_args(argv), kernel_ms=kernel_ms) == 0
    assert kernel_ms and max(kernel_ms) > 0
    for name in OUTPUTS:
        with open(os.path.join(out_dir, name), "rb") as fh:
            assert fh.read() == twin[name], name
    assert b"\tweak\n" in twin["support.tsv"] and twin["columns.tsv"].count(b"\n") > 1
