"""The host side of smx_nj under AddressSanitizer + UBSan, CPU only: the plan of a call (specimux_amd/csrc/smx_nj_plan.h)
and the kernels' bodies as host loops over the shared core (smx_nj_core.h, host build), driven by the stand-alone
tests/asan/nj_driver.cpp over buffers of exactly the planned sizes, for n = 0 .. 5, 64, 65 and 257.  Any heap / bounds / UB
report fails the test.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(REPO, "tests", "asan", "nj_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("asan") / "nj_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{REPO}/specimux_amd/csrc", DRV, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def test_nj_plan_and_bodies_under_sanitizers(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    counts = dict(zip(words[0::2], map(int, words[1::2])))
    # nine sizes x three matrices x three visiting orders; n - 3 merges for the five sizes above 3
    per_order = (4 - 3) + (5 - 3) + (64 - 3) + (65 - 3) + (257 - 3)
    assert counts["calls"] == 81 and counts["merges"] == counts["iterations"] == 9 * per_order
    assert counts["moves"] + counts["moves_none"] == counts["iterations"] and counts["moves"] >= 2000
    assert counts["moves_none"] >= 9 and counts["ties"] >= 1000
    assert counts["refusals"] == 21                 # the seven sizes with a pair, three matrices each
