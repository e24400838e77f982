"""CPU simulation of the msa call (specimux_amd/csrc/smx_msa.hip): the host plan (smx_msa_plan.h) and the three kernels as
host loops (tests/cpu/msa_host.h over smx_msa_core.h), every buffer indexed with the kernel's own expressions, the waves of
a tick, the lanes of a step and the threads of a phase visited forwards, reversed and shuffled, against a plain triple loop
-- pairs of lengths 1, 2, 15 / 16 / 17, 63 / 64 / 65, 129 and once 1025 (one row above a round of bands), 300 x 3, 3 x 300,
1 x 300, identical sequences, a deletion, repeats of one base, other bytes; trees of 3 .. 12 tips, each also under a budget
of one byte, which cuts every level into launches of one merge.  The counters it prints are bounded from below so that
its coverage cannot shrink unnoticed.  The plan's refusals are checked there and, through the library, here.  No GPU
needed."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("msa") / "msa_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "tests", "cpu"), "-o", exe,
                           os.path.join(REPO, "tests", "cpu", "msa_sim.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_msa_plan_and_kernel_loops(sim, tmp_path, seed):
    out = subprocess.run([sim, str(seed)], capture_output=True, text=True, cwd=tmp_path)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    c = {}
    for line in out.stdout.splitlines():
        key, _, val = line.partition(" ")
        if val.isdigit() and key.isidentifier():
            c[key] = int(val)
    big = seed == 1                                 # the one run with 1025 rows
    # 9 x 9 pairs twice, 3 edge shapes, 5 special cases, 10 sizes x 3 trees twice; every case in three visiting orders
    assert c["cases"] == 162 + 3 + 5 + 60 + 2 * big
    tree_merges = 3 * 2 * sum(n - 1 for n in range(3, 13))
    assert c["merges"] == 3 * (162 + 3 + 3 + 2 + 2 + 2 * big + tree_merges)
    assert c["launches"] >= c["merges"] - 3 * tree_merges // 2 and c["launches"] < c["merges"]      # levels share launches
    assert c["cells"] >= 5000000 and c["words"] >= 380000 and c["ticks"] >= 5000
    assert c["tiles"] >= 2200 and c["steps"] >= 90000 and c["edge_ops"] >= 14000
    assert c["plan_checks"] == 11 and c["refusals_checked"] == 15


def test_bad_calls_are_refused_before_the_device_is_asked():
    """Every refusal is host code alone: on a machine without a GPU the same call with good arguments is the one that
    fails, with SMX_ERR_DEVICE -- n = 0 and n = 1 included, which launch nothing but keep the calls' one order."""
    import torch
    from specimux_amd import _lib
    lib = _lib.load()
    seqs = b"ACGTACGGTACGA"
    off = np.array([0, 4, 8, 13], dtype=np.uint64)
    merges = np.array([(0, 1), (3, 2)], dtype=_lib.MSA_MERGE_DTYPE)
    rows, n_cols = np.zeros(3 * 32, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    lens, costs = np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint64)

    def call(seqs_=seqs, off_=off, n=3, merges_=merges, X=1, G=1, rows_=rows, n_cols_=n_cols, lens_=lens, costs_=costs):
        rc = lib.smx_msa(seqs_, _lib.ptr(off_), n, _lib.ptr(merges_), X, G, 32, _lib.ptr(rows_), _lib.ptr(n_cols_), _lib.ptr(lens_),
                         _lib.ptr(costs_), None)
        return rc, lib.smx_last_error().decode()
    for kw in (dict(seqs_=None), dict(off_=None), dict(merges_=None), dict(rows_=None), dict(n_cols_=None), dict(lens_=None),
               dict(costs_=None)):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_ARG and "null" in msg, (kw, rc, msg)
    for kw in (dict(X=0), dict(G=0), dict(X=1001), dict(G=1001)):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_ARG and "1..1000" in msg, (kw, rc, msg)
    rc, msg = call(off_=np.array([0, 4, 4, 13], dtype=np.uint64))
    assert rc == _lib.ERR_ARG and "sequence 1 is empty" in msg, (rc, msg)
    rc, msg = call(off_=np.array([0, 4, 8, 8 + _lib.MSA_MAX_COLS + 1], dtype=np.uint64))
    assert rc == _lib.ERR_UNSUPPORTED and "sequence 2 is longer" in msg, (rc, msg)
    rc, msg = call(n=_lib.MSA_MAX_N + 1)            # refused before the offsets are read
    assert rc == _lib.ERR_UNSUPPORTED and "4097" in msg, (rc, msg)
    for bad in ([(0, 0), (3, 2)], [(0, 3), (3, 2)], [(0, 1), (0, 2)], [(0, 1), (4, 2)]):
        rc, msg = call(merges_=np.array(bad, dtype=_lib.MSA_MERGE_DTYPE))
        assert rc == _lib.ERR_ARG and "is not one of the tree" in msg, (bad, rc, msg)
    good = _lib.OK if torch.cuda.is_available() else _lib.ERR_DEVICE
    for kw in (dict(), dict(n=0, seqs_=None, off_=None, merges_=None, rows_=None, lens_=None, costs_=None),
               dict(n=1, merges_=None, lens_=None, costs_=None)):
        rc, msg = call(**kw)
        assert rc == good, (kw, rc, msg)
    assert _lib.MSA_MAX_N == 4096 and _lib.MSA_MAX_COLS == 8192 and _lib.MSA_MERGE_DTYPE.itemsize == 8
    assert _lib.ABI_VERSION == 13 and lib.smx_abi_version() == 13
