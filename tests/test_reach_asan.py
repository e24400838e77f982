"""The host side of the bimera calls under AddressSanitizer + UBSan, CPU only: the plan of a call
(specimux_amd/csrc/smx_reach_plan.h) and the kernel as a host loop over the planned chunks (tests/cpu/reach_host.h), driven
by the stand-alone tests/asan/reach_driver.cpp over buffers of exactly the planned sizes.  Any heap / bounds / UB report
fails the test."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(REPO, "tests", "asan", "reach_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("asan") / "reach_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{REPO}/specimux_amd/csrc", f"-I{REPO}/tests/cpu", DRV, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def test_reach_plan_and_chunk_loop_under_sanitizers(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    counts = dict(zip(words[0::2], map(int, words[1::2])))
    # seven jobs (three with 1, 65 and 140 targets, one sharing the 65, one without queries, one without targets, one of
    # two twins that are each other's only target at the very end of the buffer), E = 0, 1, 7, 15
    assert counts["jobs"] == 7 and counts["plans"] == 4
    assert counts["chunks"] >= 4 * 12 and counts["items"] >= 2000 and counts["found"] >= 400 and counts["checksum"] > 0
