"""CPU simulation of the barcode survey's per-hit and per-key code (specimux_amd/csrc/smx_flank_core.h: the host/device
flank_of_hit, flank_shw and flank_take the gfx950 kernels of smx_flank.hip run, over smx_stats_core.h's table) against plain
string code: the end string built with an ordinary reverse complement and sliced, a full DP matrix for the prefix distance.
A sample of the simulation's DP distances is checked against the suite's oracle, and the counters it prints are bounded
from below so that its coverage cannot shrink unnoticed.  The host plan of smx_flank_assign (smx_flank_plan.h) runs in
the same simulation against a plain stable sort by primer.  No GPU needed."""
import os
import subprocess

import pytest

from oracle.edlib_semantics import SHW, align_c

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path_factory, name, *defines):
    exe = os.fspath(tmp_path_factory.mktemp("flank") / name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", *defines, "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", exe, os.path.join(REPO, "tests", "cpu", "flank_sim.cpp")])
    return exe


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return _build(tmp_path_factory, "flank_sim")


@pytest.fixture(scope="module")
def sim_tiny(tmp_path_factory):
    """An 8-slot local table with 2 probes: nearly every key bypasses it."""
    return _build(tmp_path_factory, "flank_sim_tiny", "-DFLANK_LCAP=8", "-DFLANK_LPROBE=2")


def run(sim, cwd, *args):
    out = subprocess.run([sim, *args], capture_output=True, text=True, cwd=cwd)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    counts = {}
    for line in out.stdout.splitlines():
        key, _, val = line.partition(" ")
        if val.lstrip("-").isdigit() and key.isidentifier():
            counts[key] = int(val)
    return counts


def test_flanks_keys_and_table_against_plain_strings(sim, tmp_path):
    c = run(sim, tmp_path, "flank")
    # S = 80 and 31, Lb = 8, 13, 23 with k = 3: every window position of the primer's end at both ends, for each of the six
    assert c["end_positions"] == 3 * 2 * (80 + 31)
    assert c["hits"] == c["pruned"] + c["short_read"] + c["short_flank"] + c["ambiguous"] + c["counted"]
    for name, least in (("pruned", 1000), ("short_read", 5000), ("short_flank", 2000), ("ambiguous", 400), ("counted", 10000)):
        assert c[name] >= least, (name, c[name])
    assert c["w26"] >= 2000                       # flanks of W = 26 bases exactly (Lb = 23)
    assert c["counted_a"] >= 5000 and c["counted_b"] >= 5000
    assert c["overlap_reads"] >= 2500             # lens of S, S + 1 and 2 S - 1: head and tail windows overlap
    assert c["repeated_keys"] >= 1000             # counts above one: the tables combine
    assert c["local_spill"] < c["counted"] // 20  # the kernel's table size holds nearly everything


def test_rows_bypass_a_tiny_local_table(sim_tiny, tmp_path):
    c = run(sim_tiny, tmp_path, "flank")
    assert c["local_spill"] >= c["counted"] * 0.9 and c["counted"] >= 10000


def test_shw_exhaustive_small(sim, tmp_path):
    c = run(sim, tmp_path, "exhaustive")
    n_cands = sum(2 ** m for m in range(1, 6))              # every {A, C} candidate of 1-5 letters
    n_flanks = sum(3 ** n for n in range(8))                # every {A, C, G} flank of 0-7 letters
    assert c["candidates"] == n_cands and c["flanks"] == n_flanks
    assert c["cases"] == n_cands * n_flanks and c["assignments"] == n_flanks * 6   # k = 0..5


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_shw_structured_random(sim, tmp_path, seed):
    c = run(sim, tmp_path, "random", str(seed))
    assert c["cases"] >= 380000
    # planted copies whose own prefix distance (DP) is exactly k, exactly k + 1
    assert c["kind_at_k"] >= 2500 and c["kind_at_k_plus_1"] >= 1500 and c["kind_exact"] >= 4000
    assert c["iupac_candidates"] >= 3000 and c["len_26"] >= 40 and c["flank_26"] >= 300 and c["ties"] >= 400
    # the simulation's reference DP against the suite's oracle
    n = 0
    with open(tmp_path / "oracle_sample.txt") as fh:
        for line in fh:
            ch, fh_, want = line.split()
            cand = bytes.fromhex(ch).decode("latin-1")
            flank = "" if fh_ == "-" else bytes.fromhex(fh_).decode("latin-1")
            got = align_c(cand, flank, SHW, -1, iupac=True)
            assert got["editDistance"] == int(want), (cand, flank, want, got["editDistance"])
            n += 1
    assert n == c["oracle_sample"] >= 300


def test_assign_plan_against_a_stable_sort_by_primer(sim, tmp_path):
    """The host plan of smx_flank_assign (smx_flank_plan.h): the candidates regrouped by primer, each group in the caller's
    order, equal a plain stable sort by primer; every refusal is refused with its message."""
    c = run(sim, tmp_path, "plan")
    assert c["plan_cases"] == 8 and c["plan_refusals"] == 16
    assert c["plan_interleaved"] >= 4            # caller's lists whose primers descend somewhere: the grouping permutes
    assert c["plan_moved"] >= 500                # candidates whose grouped slot is not their caller's index
    assert c["plan_empty_primers"] >= 5 and c["plan_primer63"] >= 500
    assert c["plan_no_candidates"] == 2 and c["plan_largest_group"] == 600 and c["plan_candidates"] >= 1500


def test_assign_checks_its_arguments_on_the_host():
    """smx_flank_assign validates keys and candidates before it touches a device."""
    import numpy as np

    from specimux_amd import _lib
    lib = _lib.load()

    def call(keys, cands, primers, k=3):
        keys = np.array(keys, dtype=np.uint64)
        off = np.zeros(len(cands) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(c) for c in cands])
        prim = np.array(primers or [0], dtype=np.uint8)
        out = [np.zeros(max(1, len(keys)), dtype=np.int32) for _ in range(3)]
        return lib.smx_flank_assign(_lib.ptr(keys), len(keys), "".join(cands).encode(), _lib.ptr(off), _lib.ptr(prim), len(cands), k,
                                    _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), None)

    assert call([], ["ACGTNRY"], [0]) == _lib.OK                       # nothing to assign: no device needed
    for cands, primers, word in ((["A" * 27], [0], "27 letters"), ([""], [0], "0 letters"), (["ACXT"], [0], "IUPAC"),
                                 (["ACGT"], [64], "primer 64")):
        assert call([], cands, primers) == _lib.ERR_ARG
        assert word in lib.smx_last_error().decode(), (word, lib.smx_last_error())
    assert call([(1 << 64) - 1], ["ACGT"], [0]) == _lib.ERR_ARG and "no flank key" in lib.smx_last_error().decode()
    assert call([27 << 52], ["ACGT"], [0]) == _lib.ERR_ARG            # a flank longer than 26 bases
    assert call([], ["ACGT"], [0], k=-1) == _lib.ERR_ARG


def _flank_create_status(tmp_path, fwd, rev, **flags):
    """smx_flank_create's status and message for a one-pool panel with these barcodes (refusals come before any device work)."""
    import ctypes as C

    from parity_utils import Both
    from specimux_amd import _lib, synth
    from specimux_amd.demultiplex import compiled_panel
    pf, sf = synth.Panel([("ITS", "ITS1F", synth.ITS1F, "ITS4", synth.ITS4)], fwd, rev).write(os.fspath(tmp_path))
    both = Both(pf, sf, **flags)
    cp = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
    lib, handle = _lib.load(), C.c_void_p()
    rc = lib.smx_flank_create(cp.handle, 1024, C.byref(handle))
    if rc == _lib.OK:
        lib.smx_flank_destroy(handle)
    return rc, lib.smx_last_error().decode()


def test_create_refuses_flanks_longer_than_a_key(tmp_path):
    from specimux_amd import _lib, synth
    f, r = synth.make_barcodes(2, 2, length=24, min_dist=8, seed=3)
    rc, msg = _flank_create_status(tmp_path, f, r, index_edit_distance=3)          # W = 27
    assert rc == _lib.ERR_UNSUPPORTED and "24 + index distance 3" in msg and "26" in msg


def test_create_refuses_barcodes_of_unequal_length(tmp_path):
    from specimux_amd import _lib, synth
    f, r = synth.make_barcodes(2, 2, seed=3)
    rc, msg = _flank_create_status(tmp_path, [f[0], f[1][:12]], r, index_edit_distance=3, disable_prefilter=True)
    assert rc == _lib.ERR_UNSUPPORTED and "not all 13 long" in msg and "12 letters" in msg
