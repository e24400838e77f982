"""CPU simulation of the primer prescan on tile codes (specimux_amd/csrc/smx_prescan_core.h: the tile-major code layout,
the tile-codes kernel's staging and copy-out, and the DP kernel's in-register bit transpose of its text) against the planes
path and a plain O(mn) dynamic program: the address function, every code dword, flag byte, flag word and match word, and the
consumer-side decode.  No GPU needed."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# partial 32-read groups, 256-read sub-tiles and 1024-read DP tiles, one read either side of each edge
READ_COUNTS = [1, 31, 32, 33, 255, 257, 1023, 1025, 2049]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("prescan_tile") / "prescan_tile_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "specimux_amd", "csrc"), "-o", exe,
                           os.path.join(REPO, "tests", "cpu", "prescan_tile_sim.cpp")])
    return exe


@pytest.mark.parametrize("n", READ_COUNTS)
@pytest.mark.parametrize("S", [16, 32, 80, 160])
def test_tile_codes_equal_planes_and_dp(sim, S, n):
    out = subprocess.run([sim, str(S), str(n), str(S + n)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 mismatches" in out.stdout
