"""The host side of the identify calls under AddressSanitizer + UBSan, CPU only: the plan of a call
(specimux_amd/csrc/smx_hits_plan.h) and the kernel as a host loop over the planned chunks (tests/cpu/hits_host.h), driven
by the stand-alone tests/asan/hits_driver.cpp over buffers of exactly the planned sizes.  Any heap / bounds / UB report
fails the test."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(REPO, "tests", "asan", "hits_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("asan") / "hits_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{REPO}/specimux_amd/csrc", f"-I{REPO}/tests/cpu", DRV, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def test_hits_plan_and_chunk_loop_under_sanitizers(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    counts = dict(zip(words[0::2], map(int, words[1::2])))
    # six jobs (three with 1, 300 and 40 targets, one sharing the 300, one without queries, one without targets), three
    # coverage bounds x three K
    assert counts["jobs"] == 6 and counts["plans"] == 9
    assert counts["chunks"] >= 9 * 10 and counts["pairs"] >= 3000 and counts["found"] >= 300 and counts["checksum"] > 0
