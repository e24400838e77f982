"""The host side of the inner-scan calls under AddressSanitizer + UBSan, CPU only: the plan of a call
(specimux_amd/csrc/smx_inner_plan.h) and the two kernels as host loops over it (tests/cpu/inner_host.h), driven by the
stand-alone tests/asan/inner_driver.cpp over buffers of exactly the planned sizes, the bases among them: they end at the
16-byte word that holds the group's last byte.  Any heap / bounds / UB report fails the test."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(REPO, "tests", "asan", "inner_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("asan") / "inner_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{REPO}/specimux_amd/csrc", f"-I{REPO}/tests/cpu", DRV, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def test_inner_plan_and_kernel_loops_under_sanitizers(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.rstrip().endswith("\n0 mismatches"), r.stdout[-2000:]
    counts = {key: int(val) for key, _, val in (line.partition(" ") for line in r.stdout.splitlines()) if key.isidentifier()}
    # the shapes of tests/cpu/inner_cases.h: Q = 1 .. 128 x margin x H x three budgets x both entries, each call compared
    # with the default budget's result
    assert counts["calls"] == counts["compared"] == 6 * 2 * 2 * 3 * 2
    assert counts["groups_one_read"] == 10 * counts["groups_default"] and counts["groups_over_budget"] > 0
    assert counts["scans_g4"] > 0 and counts["scans_g8"] > 0 and counts["scans_w32"] > 0 and counts["scans_w64"] > 0
    assert counts["passes_max"] == 16 and counts["padding_slots"] > 0 and counts["last_word_loads"] > 0
