"""CPU simulation of the clusters kernel's per-pair code (specimux_amd/csrc/smx_pairs_core.h: the host/device pairs_pair
the gfx950 kernel smx_pairs.hip runs) against a plain O(mn) DP with edlib's NW semantics, for every register class and
the generic class, with limits at the distance itself (k = d - 1, d, d + 1) and at the length difference (|m - n| = k,
k + 1).  A sample of the simulation's DP results is checked against the suite's oracle, and the counters it prints are
bounded from below so that its coverage cannot shrink unnoticed.  No GPU needed."""
import os
import subprocess

import pytest

from oracle.edlib_semantics import NW, align_c

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("pairs") / "pairs_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", exe,
                           os.path.join(REPO, "tests", "cpu", "pairs_sim.cpp")])
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


def test_pairs_exhaustive_small(sim, tmp_path):
    c = run(sim, tmp_path, "exhaustive")
    # 2^m queries (m = 1..6) x 2^n targets (n = 0..7), k = -1..max(m, n) + 1 each, register class and generic class;
    # then the empty query against targets of 0..3 bytes with five limits each
    assert c["kind_exhaustive"] == 126 * 255 and c["kind_empty_query"] == 4
    assert c["calls"] == 2 * sum(2 ** m * 2 ** n * (max(m, n) + 3) for m in range(1, 7) for n in range(8)) + 2 * 4 * 5
    assert c["k_d"] > 30000 and c["k_d_plus_1"] > 30000 and c["k_d_minus_1"] > 30000
    assert c["gap_k"] > 30000 and c["gap_k_plus_1"] > 25000


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_pairs_structured_random(sim, tmp_path, seed):
    c = run(sim, tmp_path, "random", str(seed))
    assert c["pairs"] >= 2000 and c["calls"] >= 30000
    for kind in ("point", "boundary_edits", "indel_start", "indel_end", "gap_k", "identical", "unrelated"):
        assert c["kind_" + kind] >= 280, kind
    for wr in (1, 2, 4, 8, 16):
        assert c[f"class_{wr}"] >= 40, wr
    assert c["class_0"] >= 100
    for key in ("k_d_minus_1", "k_d", "k_d_plus_1"):
        assert c[key] >= 1500, key
    assert c["gap_k"] >= 500 and c["gap_k_plus_1"] >= 300
    # the simulation's reference DP against the suite's oracle
    n = 0
    with open(tmp_path / "oracle_sample.txt") as fh:
        for line in fh:
            qh, th, k, want = line.split()
            q = bytes.fromhex(qh).decode("latin-1")
            t = bytes.fromhex(th).decode("latin-1")
            got = align_c(q, t, NW, int(k), iupac=False)["editDistance"]
            assert got == int(want), (len(q), len(t), k, want, got)
            n += 1
    assert n == c["oracle_sample"] >= 150
