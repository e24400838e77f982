"""The host side of smx_cons_profile under AddressSanitizer + UBSan, CPU only: the plan of a call with its profile tables
(specimux_amd/csrc/smx_cons_plan.h) and the kernel's body as a host loop over the shared core (smx_cons_core.h,
smx_profile_core.h, host build), driven by the stand-alone tests/asan/profile_driver.cpp over buffers of exactly the
planned sizes.  Any heap / bounds / UB report fails the test.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(REPO, "tests", "asan", "profile_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("asan") / "profile_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{REPO}/specimux_amd/csrc", DRV, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def test_profile_plan_and_core_under_sanitizers(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    counts = dict(zip(words[0::2], map(int, words[1::2])))
    # seven jobs of 1, 16, 0, 17, 4, 5 and 65 members: the last member of the four larger ones is above its limit, member 2
    # of the five with three members or more is clipped, member 3 of those with four or more is empty
    assert counts["jobs"] == 7 and counts["above"] == 4 and counts["members"] == 1 + 16 + 17 + 4 + 5 + 65 - 4
    assert counts["clipped"] == 5 and counts["empty"] == 5
    assert counts["columns"] == 63 + 15 * 64 + 16 * 127 + 4 * 128 + 4 * 129 + 64 * 100
    # every base of the 99 unclipped members once (the mutated reads are about as long as their drafts, five are empty);
    # a run per two to four draft bases and aligned member
    assert counts["q_bases"] > 8000 and counts["columns"] // 5 < counts["hp"] < counts["columns"]
