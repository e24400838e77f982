"""Every distance level of the padded barcode scan (specimux_amd/csrc/smx_barcode_core.h, bitsliced_shw_pad and the seen[]
of bitsliced_shw_pad_tails) against a plain O(M n) SHW DP over the wildcard-padded barcode: for EVERY d <= KB, not only
the lowest level, seen[d] is exactly the set of barcodes whose row-M value is d at some live column.  The diagonal
automaton of the padded scan is built on that property; tests/test_barcode_scan_cpu.py pins the lowest level and the
summary.  Every instantiation, every m = KB + 1 .. M, every ncol = 0 .. M + KB + 2, words of 1, 31 and 32 barcodes, IUPAC
barcode positions, code 15 inside the target.  One more build runs under AddressSanitizer and UBSan (host code) with
buffers of exactly the size the kernel may read.  The counters the program prints are bounded from below so that its
coverage cannot shrink unnoticed.  No GPU needed."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "cpu", "barcode_levels_sim.cpp")
INC = os.path.join(REPO, "specimux_amd", "csrc")

INST = {"pad3_8": (3, 8), "pad3_12": (3, 12), "pad3_13": (3, 13), "pad3_16": (3, 16), "pad4_13": (4, 13), "pad4_16": (4, 16),
        "tails3_8": (3, 8), "tails3_12": (3, 12), "tails3_13": (3, 13), "tails3_16": (3, 16)}
CASES = 6   # targets per (instantiation, m, word size, ncol): CASES in barcode_levels_sim.cpp


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("levels") / "barcode_levels_sim")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-Wno-unknown-pragmas", "-I", INC, "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def sim_asan(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("levels_asan") / "barcode_levels_sim_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-std=c++17", "-Wno-unknown-pragmas", "-I", INC, "-o", exe, SRC])
    return exe


def run(sim, cwd, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([sim, str(seed)], capture_output=True, text=True, cwd=cwd, env=env)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr, out.stderr[-4000:]
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    counts = {}
    for line in out.stdout.splitlines():
        key, _, val = line.partition(" ")
        if val.lstrip("-").isdigit() and key.isidentifier():
            counts[key] = int(val)
    return counts


def check_coverage(c):
    total = 0
    for inst, (kb, m_pad) in INST.items():
        # every m = KB + 1 .. M x three word sizes x every ncol = 0 .. M + KB + 2 x CASES targets
        want = (m_pad - kb) * 3 * (m_pad + kb + 3) * CASES
        assert c.get("calls_" + inst, 0) == want, (inst, c.get("calls_" + inst), want)
        total += want
    for ncol in range(0, 16 + 4 + 3):
        assert c.get(f"ncol_{ncol}", 0) >= 100, ncol
    assert c["ncol_past_scan"] >= 1000 and c["ncol_inside_barcode"] >= 5000
    words = sum(m_pad - kb for kb, m_pad in INST.values())
    assert c["words_1"] == c["words_31"] == c["words_32"] == words
    assert c["bc_iupac"] >= 500
    assert c["targets_code15"] >= total // 8 and c["targets_iupac"] >= total // 8
    # calls with a barcode exactly at level d (level 0 needs an unedited barcode inside the window; level 4 has KB = 4 only)
    for d, floor in enumerate((1000, 3000, 5000, 5000, 1000)):
        assert c[f"level_{d}_nonempty"] >= floor, d
    # the stronger property is exercised only where one barcode sits on two different levels in one call
    assert c["barcode_on_two_levels"] >= 50_000
    assert c["barcode_on_a_level"] >= 100_000 and c["barcode_on_no_level"] >= 100_000


@pytest.mark.parametrize("seed", [1, 2])
def test_barcode_levels_every_level_exact(sim, tmp_path, seed):
    check_coverage(run(sim, tmp_path, seed))


def test_barcode_levels_sanitized(sim_asan, tmp_path):
    check_coverage(run(sim_asan, tmp_path, 3))
