"""The host side of smx_msa under AddressSanitizer + UBSan, CPU only: the plan of a call (specimux_amd/csrc/smx_msa_plan.h)
and the kernels' bodies as host loops over the shared core (smx_msa_core.h, host build), driven by the stand-alone
tests/asan/msa_driver.cpp over buffers of exactly the planned sizes.  Any heap / bounds / UB report fails the test.
Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(REPO, "tests", "asan", "msa_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("asan") / "msa_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{REPO}/specimux_amd/csrc", DRV, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def test_msa_plan_and_bodies_under_sanitizers(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    counts = dict(zip(words[0::2], map(int, words[1::2])))
    # n = 0 and n = 1, ten pairs, sixteen trees whole and cut; three visiting orders each
    assert counts["calls"] == 3 * (2 + 10 + 32)
    tree_merges = 2 * 2 * sum(n - 1 for n in range(2, 10))
    assert counts["merges"] == 3 * (10 + tree_merges)
    assert counts["merges"] > counts["launches"] >= counts["merges"] - 3 * tree_merges // 2      # the whole levels share launches
    assert counts["cells"] >= 1000000 and counts["tiles"] >= 500
    assert counts["overflows"] == counts["refusals"] == 10 + 32
