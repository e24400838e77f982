"""CPU simulation of the bit-sliced barcode scans of the demux kernel's lean mode (specimux_amd/csrc/smx_barcode_core.h:
the host/device bitsliced_shw, bitsliced_shw_pad and bitsliced_shw_pad_tails the gfx950 kernel runs) against a plain
O(mn) SHW DP, barcode by barcode, for every instantiation the kernel has, every barcode length it can hold and every k.
The tables are filled by the product's bs_table_add.  The simulation runs once more under AddressSanitizer and UBSan
(host code): table blocks and target buffers are allocated at exactly the size the kernel may read.  A sample of the
simulation's DP results is checked against the suite's oracle, and the counters it prints are bounded from below so
that its coverage cannot shrink unnoticed.  No GPU needed."""
import os
import subprocess

import pytest

from oracle.edlib_semantics import SHW, align_c

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "cpu", "barcode_sim.cpp")
INC = os.path.join(REPO, "specimux_amd", "csrc")

PAD = ["pad3_8", "pad3_12", "pad3_13", "pad3_16", "pad4_13", "pad4_16", "tails3_8", "tails3_12", "tails3_13", "tails3_16"]


def _kb(inst):
    return 7 if inst == "shw8" else int(inst.split("_")[0][-1])


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("barcode") / "barcode_sim")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-Wno-unknown-pragmas", "-I", INC, "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def sim_asan(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("barcode_asan") / "barcode_sim_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-std=c++17", "-Wno-unknown-pragmas", "-I", INC, "-o", exe, SRC])
    return exe


def run(sim, cwd, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([sim, *args], capture_output=True, text=True, cwd=cwd, env=env)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr, out.stderr[-4000:]
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    counts = {}
    for line in out.stdout.splitlines():
        key, _, val = line.partition(" ")
        if val.lstrip("-").isdigit() and key.isidentifier():
            counts[key] = int(val)
    return counts


def check_instantiations(c, floor):
    for inst in PAD + ["shw8"]:
        for k in range(_kb(inst) + 1):
            assert c.get(f"calls_{inst}_k{k}", 0) >= floor, (inst, k)


def test_barcode_scan_exhaustive_small(sim, tmp_path):
    c = run(sim, tmp_path, "exhaustive")
    # m = 1..4 over 4 letters, lengths 0..m + 5; m = 5 over 3 letters, lengths 0..10
    assert c["targets"] == sum(sum(4 ** n for n in range(m + 6)) for m in range(1, 5)) + sum(3 ** n for n in range(11))
    assert c["partial_word_hits"] == c["targets"] - sum(3 ** n for n in range(11))
    # every instantiation runs with every k up to m - 1 <= 4 (bitsliced_shw<8> on targets of length <= m + k + 1)
    for inst in PAD + ["shw8"]:
        for k in range(min(_kb(inst), 4) + 1):
            assert c.get(f"calls_{inst}_k{k}", 0) >= (2500 if inst == "shw8" else 88000), (inst, k)
    assert c["summary_ties"] > 1_000_000 and c["summary_best_eq_k"] > 500_000 and c["summary_none"] > 500_000
    assert c["min_eq_k"] > 1_000_000 and c["min_eq_k_plus_1"] > 1_000_000
    assert c["tails_want_partial"] > 100_000 and c["tails_want_all"] > 100_000 and c["tails_col_found"] > 100_000


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_barcode_scan_structured_random(sim, tmp_path, seed):
    c = run(sim, tmp_path, "random", str(seed))
    assert c["hits"] == 2880
    for kind in ("edits", "cut", "interleaved", "unrelated", "exact"):
        assert c["kind_" + kind] >= 900, kind
    assert c["bc_near"] >= 800 and c["bc_iupac"] >= 200
    check_instantiations(c, 1500)
    assert c["calls_dispatched"] >= 40000
    assert c["partial_word_hits"] >= 2500
    assert c["summary_ties"] >= 10000 and c["summary_best_eq_k"] >= 10000 and c["summary_none"] >= 10000
    assert c["summary_multi_entry"] >= 40000
    assert c["tails_want_all"] >= 10000 and c["tails_want_partial"] >= 30000 and c["tails_col_found"] >= 10000
    # the simulation's reference DP against the suite's oracle: distance and the last optimal end
    n = 0
    with open(tmp_path / "oracle_sample.txt") as fh:
        for line in fh:
            bc, target, k, dist, maxend = line.split()
            k, dist, maxend = int(k), int(dist), int(maxend)
            got = align_c(bc, target, SHW, k, iupac=True)
            if dist > k:
                assert got["editDistance"] == -1, (bc, target, k, dist, got)
            else:
                assert got["editDistance"] == dist, (bc, target, k, dist, got)
                assert max(e for _, e in got["locations"]) == maxend, (bc, target, k, maxend, got)
            n += 1
    assert n == c["oracle_sample"] >= 500


@pytest.mark.parametrize("args", [("random", "1"), ("random", "3"), ("exhaustive", "3")], ids=lambda a: "-".join(a))
def test_barcode_scan_sanitized(sim_asan, tmp_path, args):
    c = run(sim_asan, tmp_path, *args)
    assert c["summary_hits"] > 1000
