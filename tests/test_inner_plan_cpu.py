"""CPU simulation of whole inner-scan calls: the plan (specimux_amd/csrc/smx_inner_plan.h: pattern tables with padding slots,
launch groups under a budget, the unit prefix, buffer sizes) and the two kernels as host loops over it
(tests/cpu/inner_host.h, the bases ending at the 16-byte word that holds the group's last byte), every output compared
(==) with the definition of a hit over the last row of the full HW recurrence (tests/cpu/inner_cases.h), and across budgets
and entries.  The counters the simulation prints are asserted.  No GPU needed."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (1, 4, 5, 8, 9, 128)
N_READS = 10                       # lengths 0, 1, 2 margin, 2 margin + 1, 2 margin + PL, 2 margin + PL + 1, 20 000 and three more


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("inner_plan") / "inner_plan_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "tests", "cpu"), "-o", exe, os.path.join(REPO, "tests", "cpu", "inner_plan_sim.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    return {key: int(val) for key, _, val in (line.partition(" ") for line in out.stdout.splitlines()) if key.isidentifier()}


def test_every_output_equals_the_definition_whatever_the_budget(counts):
    c = counts
    settings = len(QS) * 2 * 2                       # Q x margin (0, 80) x H (1, 8)
    assert c["calls"] == settings * 3 * 2            # x budget (default, one read per group, less than the longest read) x entry
    # per call one comparison with the default budget's result and one per (read, pattern) with the definition
    assert c["compared"] == c["calls"] + 3 * 2 * 2 * 2 * N_READS * sum(QS)
    assert c["merges"] == 3 * 2 * 2 * 2 * N_READS * sum(QS)
    assert c["runs"] > 100000 and c["more_than_H"] > 500


def test_the_shapes_reach_every_table_layout_and_grouping(counts):
    c = counts
    settings = len(QS) * 2 * 2
    # the default budget keeps the ten reads in one group, a budget of one byte puts each in its own, and 10 000 bytes
    # (less than the read of 20 000 bases) is between the two
    assert c["groups_default"] == settings * 2 and c["groups_one_read"] == settings * 2 * N_READS
    assert c["groups_default"] < c["groups_small"] < c["groups_one_read"]
    assert c["groups_over_budget"] >= settings * 2 * 2 and c["groups_of_one"] > c["groups_one_read"]
    # G = 4 and G = 8, 32- and 64-bit words, 1 to 16 passes, padding slots, and loads of the last 16-byte word of the bases
    assert c["scans_g4"] > 0 and c["scans_g8"] > 0 and c["scans_w32"] > 0 and c["scans_w64"] > 0
    assert c["passes_max"] == 16 and c["padding_slots"] > 0 and c["last_word_loads"] > 0
    assert c["units"] > 5000 and c["scans"] > c["units"]
