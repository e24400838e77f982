"""CPU simulation of the tree call (specimux_amd/csrc/smx_nj.hip): the host plan (smx_nj_plan.h) and the three kernels as
host loops (tests/cpu/nj_host.h over smx_nj_core.h, compiled with -ffp-contract=off), the row-minimum and the global
reduction and the threads of the join's phases visited forwards, reversed and shuffled, against a plain triple loop --
n = 0 .. 9, 63, 64, 65, 100, 255, 256, 257 and once 1030 (more than one slot per join thread); random, narrow (many equal
Q), all-equal, zero, ladder and 2^31 - 1 matrices.  The counters it prints are bounded from below so that its coverage
cannot shrink unnoticed.  The plan's refusals and the answers of n <= 3 are checked there and, through the library,
here.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("nj") / "nj_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "tests", "cpu"), "-o", exe,
                           os.path.join(REPO, "tests", "cpu", "nj_sim.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_nj_plan_and_kernel_loops(sim, tmp_path, seed):
    out = subprocess.run([sim, str(seed)], capture_output=True, text=True, cwd=tmp_path)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    c = {}
    for line in out.stdout.splitlines():
        key, _, val = line.partition(" ")
        if val.isdigit() and key.isidentifier():
            c[key] = int(val)
    big = seed == 1                                 # the one run with n = 1030
    assert c["cases"] == 97 + big                   # 17 sizes x 6 matrices, less 2^31 - 1 above n = 64: 4 sizes
    per_order = sum(max(n - 3, 0) for n in (list(range(10)) + [63, 64, 65, 100, 255, 256, 257]) for _ in range(5)) \
        + sum(max(n - 3, 0) for n in (list(range(10)) + [63, 64]))
    assert c["merges_checked"] == c["iterations"] == 3 * (per_order + 1027 * big)
    assert c["moves"] + c["moves_none"] == c["iterations"]
    assert c["moves"] >= 14000 and c["moves_none"] >= 1500          # hi != na - 1 and hi == na - 1
    assert c["ties"] >= 500000                                       # equal Q met in the global reduction
    assert c["rowmin_rows"] >= 1500000 and c["rowmin_entries"] >= 100000000 and c["join_slots"] >= 1500000
    assert c["refusals_checked"] == 7


def test_bad_calls_are_refused_before_the_device_is_asked():
    """Every refusal is host code alone: on a machine without a GPU the same call with good arguments is the one that
    fails, with SMX_ERR_DEVICE -- n <= 3 included, which launches nothing but keeps the calls' one order."""
    import torch
    from specimux_amd import _lib
    lib = _lib.load()
    tri = np.arange(1, 11, dtype=np.int32)          # n = 5
    merges = np.zeros(8, dtype=_lib.NJ_MERGE_DTYPE)
    last, last_d = np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.float64)

    def call(tri_, n, merges_=merges, last_=last, last_d_=last_d):
        rc = lib.smx_nj(_lib.ptr(tri_), n, _lib.ptr(merges_), _lib.ptr(last_), _lib.ptr(last_d_), None)
        return rc, lib.smx_last_error().decode()
    for args, word in (((None, 5), "null"), ((tri, 5, None), "null"), ((tri, 5, merges, None), "null"),
                       ((tri, 5, merges, last, None), "null"), ((None, 2), "null")):
        rc, msg = call(*args)
        assert rc == _lib.ERR_ARG and word in msg, (args, rc, msg)
    bad = tri.copy()
    bad[7] = -1
    rc, msg = call(bad, 5)
    assert rc == _lib.ERR_ARG and "distance 7 is negative" in msg, (rc, msg)
    rc, msg = call(bad, 4)                          # six entries: the seventh is not the call's
    assert rc == (_lib.OK if torch.cuda.is_available() else _lib.ERR_DEVICE), msg
    rc, msg = call(tri, _lib.NJ_MAX_N + 1)          # refused before the triangle is read
    assert rc == _lib.ERR_UNSUPPORTED and "16385" in msg, (rc, msg)
    for n in (0, 1, 2, 3, 5):                       # good calls; without merges where there are none
        rc, msg = call(tri if n >= 2 else None, n, merges if n > 3 else None)
        assert rc == (_lib.OK if torch.cuda.is_available() else _lib.ERR_DEVICE), (n, msg)
    assert _lib.NJ_MAX_N == 16384 and _lib.NJ_MERGE_DTYPE.itemsize == 40
    assert _lib.ABI_VERSION == 13 and lib.smx_abi_version() == 13
