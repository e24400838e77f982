"""CPU simulation of the inner scan's per-lane code (specimux_amd/csrc/smx_inner_core.h: the host/device inner_scan_piece
and inner_merge the gfx950 kernels of smx_inner.hip run) against a plain last-row DP and the definition of a hit applied to
the whole read: exhaustively over small alphabets, and on structured random cases at every piece length the kernel can
choose and two it cannot.  A sample of the simulation's DP minima is checked against the suite's oracle, and the counters
it prints are bounded from below so that its coverage cannot shrink unnoticed.  No GPU needed."""
import os
import subprocess

import pytest

from oracle.edlib_semantics import HW, align_c

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("inner") / "inner_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(REPO, "specimux_amd", "csrc"), "-o", exe,
                           os.path.join(REPO, "tests", "cpu", "inner_sim.cpp")])
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


def test_inner_exhaustive_small(sim, tmp_path):
    c = run(sim, tmp_path, "exhaustive")
    n_reads = sum(3 ** n for n in range(10))
    n_slots = sum(2 ** m * m for m in range(1, 6))       # every {A, C} pattern of length 1-5 with every valid k
    assert c["patterns"] == n_slots and c["reads"] == n_reads
    assert c["cases"] == n_slots * n_reads * 4 * 2         # margins 0-3, H = 1 and 3
    # every case at the kernel's piece length (6 calls of up to 43 slots per read, margin and H), a quarter again in tiny pieces
    assert c["scans"] >= 6 * n_reads * 4 * 2 * 1.2
    assert c["units"] > 10_000_000 and c["runs"] > 50_000_000


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_inner_structured_random(sim, tmp_path, seed):
    c = run(sim, tmp_path, "random", str(seed))
    assert c["cases"] >= 3000 and c["scans"] == 6 * 288 and c["runs"] >= 20000
    for pl in (64, 128, 256, 512, 37, 100):                # the kernel's four piece lengths and two off its grid
        assert c[f"pl_{pl}"] == 288, pl
    for kind in ("touching", "one_apart", "exact"):
        assert c["kind_" + kind] >= 500, kind
    # planted copies whose own best distance (DP on the copy) is exactly k, exactly k + 1
    assert c["kind_at_k"] >= 250 and c["kind_at_k_plus_1"] >= 250
    assert c["class_32"] >= 8000 and c["class_64"] >= 5000
    assert c["more_than_H"] >= 200 and c["runs_across_boundary"] >= 2000
    # the simulation's reference DP against the suite's oracle: best distance and the first column that attains it
    n = 0
    with open(tmp_path / "oracle_sample.txt") as fh:
        for line in fh:
            ph, th, want, end = line.split()
            p, t = bytes.fromhex(ph).decode("latin-1"), bytes.fromhex(th).decode("latin-1")
            got = align_c(p, t, HW, -1, iupac=True)
            assert got["editDistance"] == int(want), (p, len(t), want, got["editDistance"])
            assert got["locations"][0][1] == int(end), (p, len(t), end, got["locations"][:2])
            n += 1
    assert n == c["oracle_sample"] >= 150
