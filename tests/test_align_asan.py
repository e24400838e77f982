"""The alignment kernels' lane bodies under AddressSanitizer + UBSan, CPU only: specimux_amd/csrc/smx_align_lane.h compiled
for the host (tests/cpu/align_host.h) and driven by the stand-alone tests/asan/align_driver.cpp over buffers of exactly the
sizes smx_align and smx_align_batch allocate.  Any heap / bounds / UB report fails the test."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(REPO, "tests", "asan", "align_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("asan") / "align_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{REPO}/specimux_amd/csrc", f"-I{REPO}/tests/cpu", DRV, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def test_alignment_lanes_under_sanitizers(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.rstrip().endswith("\n0 mismatches"), r.stdout[-2000:]
    counts = {key: int(val) for key, _, val in (line.partition(" ") for line in r.stdout.splitlines()) if key.isidentifier()}
    # the sets of tests/cpu/align_sim.cpp (tests/test_align_cpu.py derives the figures): the exhaustive set's 120 queries x
    # 21 844 targets x 2 modes x 6 k, the 199 targets that wrap a byte-wide score by construction, k >= m in both
    assert counts["cases"] == 120 * sum(4 ** n for n in range(1, 8)) * 2 * 6 and counts["queries_refused"] == 220
    assert counts["full_prefix_cases"] == 199 and counts["wrap_witnesses"] >= 199
    assert counts["single_cases"] == 4464 and counts["batch_cases"] == 3824 and counts["wrap_k_ge_m"] == 3200
    assert counts["cap_zero_launches"] >= 1440 + 60 and counts["dirty_workspace_launches"] >= 1440 + 30
