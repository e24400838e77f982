"""The host side of smx_cons_phase under AddressSanitizer + UBSan, CPU only: the plan of a call with its variant tables
(specimux_amd/csrc/smx_cons_plan.h) and the shared core (smx_cons_core.h, smx_phase_core.h, host build), driven by the
stand-alone tests/asan/phase_driver.cpp over buffers of exactly the planned sizes.  Any heap / bounds / UB report fails
the test.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(REPO, "tests", "asan", "phase_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("asan") / "phase_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{REPO}/specimux_amd/csrc", DRV, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def test_phase_plan_and_core_under_sanitizers(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    counts = dict(zip(words[0::2], map(int, words[1::2])))
    # five jobs with members and one without, under max_sites = 1, 3 and 64: the planted allele has three sites and the
    # noise a few more, so the two small tables clip every job that has one
    assert counts["jobs"] == 6 and counts["kept"] >= 4 * (1 + 3 + 3) and counts["clipped"] >= 8
    assert counts["bits"] > 1000 and counts["checksum"] > 0
