"""CPU simulation of whole specimine calls: the plan (specimux_amd/csrc/smx_mine_plan.h) and the kernel as a host loop over
the planned chunks (tests/cpu/mine_host.h, the first record of every workgroup found by chunk_owner's search over 64 emulated
lanes), every distance and best identity compared (==) with the full-matrix HW recurrence of tests/cpu/mine_plan_sim.cpp.
The counters the simulation prints are asserted, so that a shape that stops reaching a class, a second chunk or the capped
grid fails.  No GPU needed."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("mine_plan") / "mine_plan_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "tests", "cpu"), "-o", exe, os.path.join(REPO, "tests", "cpu", "mine_plan_sim.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    return {key: int(val) for key, _, val in (line.partition(" ") for line in out.stdout.splitlines()) if key.isidentifier()}


def test_every_output_equals_the_plain_dp(counts):
    c = counts
    # four limit variants (-1, 0, m / 10, above m, rotating over the queries) x the production budget and one slice
    assert c["plans"] == 8 and c["capped_plans"] == 4
    # jobs: 2 x (11 queries x 300 targets) + 3 x 1 + 3 x 127 + 3 x 128 + 3 x 129 + 2 x 2; a best identity per job target
    pairs = 2 * 11 * 300 + 3 * 1 + 3 * 127 + 3 * 128 + 3 * 129 + 2 * 2
    best = 2 * 300 + 1 + 127 + 128 + 129 + 10 + 2
    assert c["pairs"] == 8 * pairs and c["compared"] == 8 * (pairs + best)
    assert c["within"] > 30000 and c["beyond"] > 20000 and c["best_set"] > 4000
    assert c["ref_pairs"] > 3500


def test_the_shapes_reach_every_class_and_the_chunk_walk(counts):
    c = counts
    for cls in range(6):
        assert c[f"class_pairs_{cls}"] > 5000 and c[f"class_blocks_{cls}"] >= 8, cls
    # records of two and three chunks, workgroups that start inside a record, tables shared by the records of a query
    assert c["records"] == 8 * (2 * 11 + 4 * 3 + 2) and c["records_two_chunks"] >= 8 * 22
    assert c["blocks_inside"] >= 8 and c["builds"] < c["records"] < c["chunks"]
    # with a budget of one slice the generic class is one workgroup: 4 of the 8 plans have 2 blocks there, 4 have 1
    assert c["class_blocks_0"] == 4 * 2 + 4 * 1


def test_owner_search_takes_up_to_four_rounds(counts):
    # prefixes of 1 .. 300 001 records: the 64-lane search against std::upper_bound, a fourth round from 262 145 records on
    assert counts["owner_sweep_rounds"] == 4 and counts["owner_sweep_searches"] > 5000
