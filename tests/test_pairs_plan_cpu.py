"""CPU simulation of whole clusters calls: the plan (specimux_amd/csrc/smx_pairs_plan.h), the kernel as a host loop over the
planned chunks (tests/cpu/pairs_host.h: a row's first chunk, the packed-triangle index, one ballot per 64 lanes with the two
guarded word stores) and the mirror of the triangle, every distance and adjacency word compared (==) with the full-matrix
NW recurrence of tests/cpu/pairs_plan_sim.cpp.  The counters the simulation prints are asserted.  No GPU needed."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (33, 0, 257, 1, 128, 2, 31, 129, 32, 127)           # the jobs of tests/cpu/pairs_cases.h


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("pairs_plan") / "pairs_plan_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "tests", "cpu"), "-o", exe, os.path.join(REPO, "tests", "cpu", "pairs_plan_sim.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    return {key: int(val) for key, _, val in (line.partition(" ") for line in out.stdout.splitlines()) if key.isidentifier()}


def test_every_output_equals_the_plain_dp(counts):
    c = counts
    pairs = sum(n * (n - 1) // 2 for n in SIZES)
    words = sum(n * ((n + 31) // 32) for n in SIZES)
    # two limit variants (none; mixed) x the production budget and one slice, both modes each
    assert c["plans"] == 4 and c["capped_plans"] == 2 and c["refused_overlap"] == 1
    assert c["ref_pairs"] == pairs and c["pairs"] == 4 * pairs and c["compared"] == 4 * (pairs + words)
    assert c["within"] > 100000 and c["beyond"] > 30000 and c["neighbours"] == c["within"]


def test_the_shapes_reach_every_class_and_the_triangle_edges(counts):
    c = counts
    for cls in range(6):
        assert c[f"class_pairs_{cls}"] > 4000, cls
    rows = sum(max(n - 1, 0) for n in SIZES)
    # from n = 128 on the rows 127 .. n - 2 start behind chunk 0 (a job's last read has no row): 129 + 0 + 1 of them
    late = sum(max(n - 1 - 127, 0) for n in SIZES)
    assert c["rows"] == 4 * rows and c["rows_late"] == 4 * late and late == 130
    # a table is rebuilt where a workgroup starts inside a row, so there are more builds than rows, fewer than chunks
    assert c["blocks_inside"] > 100 and c["owner_rounds_max"] == 2 and c["rows"] < c["builds"] < c["chunks"]
    # neighbours mode: two words per wave and chunk, less what the guards w0 < nw and w0 + 1 < nw hold back
    assert c["word_stores"] + c["words_guarded"] == 4 * c["chunks"] and c["words_guarded"] > 1000
