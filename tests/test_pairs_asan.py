"""The host side of the clusters calls under AddressSanitizer + UBSan, CPU only: the plan of a call
(specimux_amd/csrc/smx_pairs_plan.h, with the mirror of the adjacency triangle) and the kernel as a host loop over the planned
chunks (tests/cpu/pairs_host.h), driven by the stand-alone tests/asan/pairs_driver.cpp over buffers of exactly the planned
sizes.  Any heap / bounds / UB report fails the test."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(REPO, "tests", "asan", "pairs_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("asan") / "pairs_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{REPO}/specimux_amd/csrc", f"-I{REPO}/tests/cpu", DRV, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def test_pairs_plan_and_chunk_loop_under_sanitizers(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.rstrip().endswith("\n0 mismatches"), r.stdout[-2000:]
    counts = {key: int(val) for key, _, val in (line.partition(" ") for line in r.stdout.splitlines()) if key.isidentifier()}
    # the shapes of tests/cpu/pairs_cases.h: jobs of 0 .. 257 reads, two limit variants x the production budget and one
    # slice of scratch, every class, rows that start behind chunk 0, guarded word stores
    assert counts["plans"] == 4 and counts["capped_plans"] == 2 and counts["pairs"] == 4 * 58771
    assert all(counts[f"class_pairs_{c}"] > 4000 for c in range(6))
    assert counts["rows_late"] == 4 * 130 and counts["words_guarded"] > 1000 and counts["neighbours"] > 100000
