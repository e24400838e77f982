"""The primer DP's column bookkeeping on the CPU (tests/cpu/prescan_pair_sim.cpp over specimux_amd/csrc/smx_prescan_core.h):
the single-ripple gap counter against the two-ripple one, transpose32 in both forms against its definition, and the DP
against a plain O(mn) dynamic program at the window lengths and primer lengths where a column pair, a chunk boundary or
an inert row can go wrong.  No GPU needed."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("prescan_pair") / "prescan_pair_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "specimux_amd", "csrc"), "-o", exe,
                           os.path.join(REPO, "tests", "cpu", "prescan_pair_sim.cpp")])
    return exe


def test_counter_and_transpose(sim):
    out = subprocess.run([sim, "unit"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "unit: 0 mismatches" in out.stdout


# S = 16: one chunk (the pair behind the prologue and the last pair of the run); S = 32: a pair boundary on a chunk boundary
@pytest.mark.parametrize("mr", [22, 24, 31])
@pytest.mark.parametrize("s", [16, 32])
def test_dp_equals_plain_dp(sim, s, mr):
    out = subprocess.run([sim, "dp", str(s), str(mr), str(100 + s + mr)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 mismatches" in out.stdout
