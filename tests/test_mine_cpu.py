"""CPU simulation of the specimine kernel's per-pair code (specimux_amd/csrc/smx_mine_core.h: the host/device mine_pair the
gfx950 kernel smx_mine.hip runs) against a plain O(mn) DP with edlib's HW semantics, for every register class and the
generic class, with limits at the distance itself (k = d - 1, d, d + 1).  A sample of the simulation's DP results is
checked against the suite's oracle, and the counters it prints are bounded from below so that its coverage cannot
shrink unnoticed.  No GPU needed."""
import os
import subprocess

import pytest

from oracle.edlib_semantics import HW, align_c

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("mine") / "mine_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", exe,
                           os.path.join(REPO, "tests", "cpu", "mine_sim.cpp")])
    return exe


def run(sim, cwd, *args):
    out = subprocess.run([sim, *args], capture_output=True, text=True, cwd=cwd)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    counts = {}
    for line in out.stdout.splitlines():
        key, _, val = line.partition(" ")
        if val.lstrip("-").isdigit() and key.isidentifier():
            counts[key] = int(val)
    return counts


def test_mine_exhaustive_small(sim, tmp_path):
    c = run(sim, tmp_path, "exhaustive")
    # sum over m = 1..6 of 2^m queries x (2^8 - 1) targets; k = -1..m + 1 each, register class and generic class
    assert c["pairs"] == 126 * 255
    assert c["calls"] == 2 * 255 * sum(2 ** m * (m + 3) for m in range(1, 7))
    assert c["k_d"] == c["k_d_plus_1"] > 30000 and c["k_d_minus_1"] > 25000


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mine_structured_random(sim, tmp_path, seed):
    c = run(sim, tmp_path, "random", str(seed))
    assert c["pairs"] >= 2200 and c["calls"] >= 30000
    for kind in ("point", "boundary_edits", "long_indel", "tandem", "flanked", "unrelated", "short"):
        assert c["kind_" + kind] >= 300, kind
    for wr in (1, 2, 4, 8, 16):
        assert c[f"class_{wr}"] >= 40, wr
    assert c["class_0"] >= 100
    for key in ("k_d_minus_1", "k_d", "k_d_plus_1"):
        assert c[key] >= 2000, key
    # the simulation's reference DP against the suite's oracle
    n = 0
    with open(tmp_path / "oracle_sample.txt") as fh:
        for line in fh:
            qh, th, k, want = line.split()
            q = bytes.fromhex(qh).decode("latin-1")
            t = "" if th == "-" else bytes.fromhex(th).decode("latin-1")
            got = align_c(q, t, HW, int(k), iupac=False)["editDistance"]
            assert got == int(want), (len(q), len(t), k, want, got)
            n += 1
    assert n == c["oracle_sample"] >= 150
