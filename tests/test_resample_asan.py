"""The host side of smx_cons_resample under AddressSanitizer + UBSan, CPU only: the plan of a call with its resampling
tables (specimux_amd/csrc/smx_cons_plan.h) and the kernel's body as a host loop over the shared core (smx_cons_core.h,
smx_resample_core.h, host build), driven by the stand-alone tests/asan/resample_driver.cpp over buffers of exactly the
planned sizes.  Any heap / bounds / UB report fails the test.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(REPO, "tests", "asan", "resample_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("asan") / "resample_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{REPO}/specimux_amd/csrc", DRV, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def test_resample_plan_and_core_under_sanitizers(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    counts = dict(zip(words[0::2], map(int, words[1::2])))
    # five jobs with members and one without, under 1, 3 and 16 levels: every agree word of every level is visited
    # (drafts of 40 + n % 7 bases), the planted allele clears bits and the last member of each larger job has no row
    drafts = [40 + n % 7 for n in (1, 63, 0, 64, 65, 129)]
    assert counts["jobs"] == 6 and counts["words"] == (1 + 3 + 16) * sum(m + 1 for m in drafts)
    assert counts["set"] > counts["clear"] > 1000 and counts["voters"] > 100000 and counts["above"] == 4
