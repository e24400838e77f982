"""CPU simulation of the consensus kernel's per-pair code (specimux_amd/csrc/smx_cons_core.h: the host/device cons_pair
the gfx950 kernel smx_cons.hip runs) against a plain O(mn) DP whose full matrix is walked back by the fixed rule
(diagonal, else up, else left): distances and pileup rows identical word for word, for every register class and the
generic class, over a reused, never cleared history.  Every reference row is also replayed on its draft (it rebuilds
the read) and its edits are counted (they add up to the distance).  A sample of the simulation's DP distances is
checked against the suite's oracle, and the counters it prints are bounded from below so that its coverage cannot
shrink unnoticed.  No GPU needed."""
import os
import subprocess

import pytest

from oracle.edlib_semantics import NW, align_c

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("cons") / "cons_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", exe, os.path.join(REPO, "tests", "cpu", "cons_sim.cpp")])
    return exe


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


def test_cons_exhaustive_small(sim, tmp_path):
    c = run(sim, tmp_path, "exhaustive")
    # 2^m drafts (m = 1..6) x 2^n reads (n = 0..7), k = -1..max(m, n) + 1 each, register class and generic class
    assert c["kind_exhaustive"] == 126 * 255
    assert c["calls"] == 2 * sum(2 ** m * 2 ** n * (max(m, n) + 3) for m in range(1, 7) for n in range(8))
    assert c["rows_equal"] > 400000                        # the calls within their limit
    assert c["replayed"] > 31000 and c["edit_counted"] == 126 * 255
    assert c["k_d"] > 30000 and c["k_d_plus_1"] > 30000 and c["k_d_minus_1"] > 30000
    assert c["gap_k"] > 30000 and c["gap_k_plus_1"] > 25000
    assert c["ins_len_4"] > 500 and c["ins_len_5"] > 200


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_cons_structured_random(sim, tmp_path, seed):
    c = run(sim, tmp_path, "random", str(seed))
    assert c["pairs"] >= 1700 and c["calls"] >= 25000 and c["rows_equal"] >= 18000
    for kind in ("point", "boundary_edits", "indel_start", "indel_end", "gap_k", "identical", "unrelated", "ins_clip",
                 "homopolymer", "band_top"):
        assert c["kind_" + kind] >= 170, kind
    for wr in (1, 2, 4, 8, 16):
        assert c[f"class_{wr}"] >= 60, wr
    assert c["class_0"] >= 100
    for key in ("k_d_minus_1", "k_d", "k_d_plus_1"):
        assert c[key] >= 1400, key
    assert c["gap_k"] >= 500 and c["gap_k_plus_1"] >= 300
    assert c["ins_len_4"] >= 1000 and c["ins_len_5"] >= 800 and c["ins_len_clipped"] >= 10   # the slot and length clips
    assert c["band_top_dropped"] >= 5000 and c["band_bottom_joined"] >= 5000   # blocks left at the top, joined below
    assert c["replayed"] >= 500 and c["edit_counted"] >= 800
    # the simulation's reference DP against the suite's oracle
    n = 0
    with open(tmp_path / "oracle_sample.txt") as fh:
        for line in fh:
            qh, th, k, want = line.split()
            q = bytes.fromhex(qh).decode("latin-1")
            t = bytes.fromhex(th).decode("latin-1")
            got = align_c(q, t, NW, int(k), iupac=False)["editDistance"]
            assert got == int(want), (len(q), len(t), k, want, got)
            n += 1
    assert n == c["oracle_sample"] >= 150


def test_bad_jobs_are_refused_before_the_device_is_asked():
    """An empty draft, overlapping member ranges and indices out of range are SMX_ERR_ARG from host code alone: on a
    machine without a GPU the same call with good jobs is the one that fails, with SMX_ERR_DEVICE."""
    import numpy as np
    import torch
    from specimux_amd import _lib, calls
    lib = _lib.load()
    reads = [b"ACGTACGT", b"ACGAACGT", b"", b"ACGT", b"ACGTT"]
    roff = calls.offsets(reads)
    ks = np.array([2] * len(reads), dtype=np.int32)

    def call(jobs, fn):
        jarr = np.array(jobs, dtype=_lib.CONS_JOB_DTYPE)
        a, b = np.zeros(4096, dtype=np.uint32), np.zeros(64, dtype=np.int32)
        rc = fn(b"".join(reads), _lib.ptr(roff), len(reads), _lib.ptr(ks), _lib.ptr(jarr), len(jobs), _lib.ptr(a), _lib.ptr(b), None)
        return rc, lib.smx_last_error().decode()
    for fn in (lib.smx_cons_pileup, lib.smx_cons_votes):
        rc, msg = call([(2, 0, 2)], fn)
        assert rc == _lib.ERR_ARG and "empty draft" in msg
        rc, msg = call([(0, 0, 3), (3, 2, 2)], fn)
        assert rc == _lib.ERR_ARG and "overlap" in msg
        rc, msg = call([(5, 0, 2)], fn)
        assert rc == _lib.ERR_ARG and "out of bounds" in msg
        rc, msg = call([(0, 3, 3)], fn)
        assert rc == _lib.ERR_ARG and "out of bounds" in msg
        rc, msg = call([(0, 0, 2), (3, 2, 0), (0, 2, 3)], fn)   # touching ranges, a shared draft, an empty job: good
        assert rc == (_lib.OK if torch.cuda.is_available() else _lib.ERR_DEVICE), msg
