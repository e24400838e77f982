"""The host side of smx_flank_assign under AddressSanitizer + UBSan, CPU only: the plan of a call
(specimux_amd/csrc/smx_flank_plan.h -- argument checks and the candidates regrouped by primer) driven by the stand-alone
tests/asan/flank_driver.cpp over arguments of exactly the sizes the call names.  Any heap / bounds / UB report fails the
test."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(REPO, "tests", "asan", "flank_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("asan") / "flank_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{REPO}/specimux_amd/csrc", f"-I{REPO}/tests/cpu", DRV, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def test_flank_assign_plan_under_sanitizers(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.rstrip().endswith("\n0 mismatches"), r.stdout[-2000:]
    words = r.stdout.split()
    counts = dict(zip(words[0::2], words[1::2]))
    assert int(counts["plan_cases"]) == 8 and int(counts["plan_refusals"]) == 16
    assert int(counts["plan_largest_group"]) == 600 and int(counts["plan_no_candidates"]) == 2
