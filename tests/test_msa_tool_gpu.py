"""specimux_amd.msa on the GPU: the tool over a 24-sequence, three-group run with its three device calls
(smx_pairs_distances, smx_nj, smx_msa) writes the same bytes as the run with the twins, with and without --split."""
import pytest

import tree_utils as TU
from specimux_amd import msa
from test_msa_cpu import TWINS, run_tool

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("split", [False, True])
def test_the_tool_with_the_device_calls(tmp_path, split):
    names, seqs = TU.synthetic_plate(seed=29, groups=3, per_group=8)
    seen = []

    def msa_fn(group, merges, *rest):
        seen.append(len(group))
        return msa.calls.msa(group, merges, *rest)

    def extra(tag):
        return ["--split", "0.05", "--groups-dir", tmp_path / f"{tag}.groups"] if split else ["--fasta-out", tmp_path / f"{tag}.aln"]
    device = run_tool(tmp_path, names, seqs, "device", extra("device") + ["--mismatch", 2, "--gap", 3], msa_fn=msa_fn)
    twin = run_tool(tmp_path, names, seqs, "twin", extra("twin") + ["--mismatch", 2, "--gap", 3], **TWINS)
    assert device == twin
    # one call over the run, or one per group of two or more (the root may lie inside a planted group and split it)
    assert seen == [24] if not split else (len(seen) >= 2 and min(seen) >= 2 and sum(seen) <= 24)
    assert set(device) == ({"report", "columns", "json", "groups"} if split else {"report", "columns", "json", "fasta"})
