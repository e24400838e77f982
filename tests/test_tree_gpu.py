"""specimux_amd.tree on the GPU: the tool over the small synthetic plate with its two device calls (smx_pairs_distances,
smx_nj) writes the same bytes as the run with the twins of tests/tree_utils.py."""
import numpy as np
import pytest

import tree_utils as U
from specimux_amd import tree
from test_tree_cpu import run_tool

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("extra", [(), ("--no-negative", "--max-distance", "0.10")])
def test_the_tool_with_the_device_calls(tmp_path, extra):
    names, seqs = U.synthetic_plate(seed=23, groups=3, per_group=5)
    ms = []
    args_seen = {}

    def nj_fn(tri, n, kernel_ms=None):
        args_seen["n"] = n
        return tree.calls.nj(tri, n, kernel_ms)

    device = run_tool(tmp_path, names, seqs, "device", extra, nj_fn=nj_fn)
    twin = run_tool(tmp_path, names, seqs, "twin", extra, edits_fn=U.edits_twin, nj_fn=U.nj_twin)
    assert args_seen["n"] == 15
    for kind in ("newick", "report", "json"):
        assert device[kind] == twin[kind], kind
    assert len(U.read_newick(device["newick"].decode())) == 2 * 15 - 3


def test_the_device_distances_are_the_twin_s():
    names, seqs = U.synthetic_plate(seed=5, groups=2, per_group=3, length=90)
    enc = [s.encode() for s in seqs]
    ks = tree.limits_of(enc, 0.30)
    assert np.array_equal(tree.device_edits(enc, ks), U.edits_twin(enc, ks))
