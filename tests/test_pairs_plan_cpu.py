"""CPU simulation of whole clusters calls: the plan (specimux_amd/csrc/smx_pairs_plan.h), the kernel as a host loop over the
planned chunks (tests/cpu/pairs_host.h: a row's first chunk, the packed-triangle index, one ballot per 64 lanes with the two
guarded word stores) and the mirror of the triangle, every distance and adjacency word compared (==) with the full-matrix
NW recurrence of tests/cpu/pairs_plan_sim.cpp.  The counters the simulation prints are asserted.  No GPU needed."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (33, 0, 257, 1, 128, 2, 31, 129, 32, 127)           # the jobs of tests/cpu/pairs_cases.h


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("pairs_plan") / "pairs_plan_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "tests", "cpu"), "-o", exe, os.path.join(REPO, "tests", "cpu", "pairs_plan_sim.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    return {key: int(val) for key, _, val in (line.partition(" ") for line in out.stdout.splitlines()) if key.isidentifier()}


def test_every_output_equals_the_plain_dp(counts):
    c = counts
    pairs = sum(n * (n - 1) // 2 for n in SIZES)
    words = sum(n * ((n + 31) // 32) for n in SIZES)
    # two limit variants (none; mixed) x the production budget and one slice, both modes each
    assert c["plans"] == 4 and c["capped_plans"] == 2 and c["refused_overlap"] == 1
    assert c["ref_pairs"] == pairs and c["pairs"] == 4 * pairs and c["compared"] == 4 * (pairs + words)
    assert c["within"] > 100000 and c["beyond"] > 30000 and c["neighbours"] == c["within"]


def test_the_shapes_reach_every_class_and_the_triangle_edges(counts):
    c = counts
    for cls in range(6):
        assert c[f"class_pairs_{cls}"] > 4000, cls
    rows = sum(max(n - 1, 0) for n in SIZES)
    # from n = 128 on the rows 127 .. n - 2 start behind chunk 0 (a job's last read has no row): 129 + 0 + 1 of them
    late = sum(max(n - 1 - 127, 0) for n in SIZES)
    assert c["rows"] == 4 * rows and c["rows_late"] == 4 * late and late == 130
    # a table is rebuilt where a workgroup starts inside a row, so there are more builds than rows, fewer than chunks
    assert c["blocks_inside"] > 100 and c["owner_rounds_max"] == 2 and c["rows"] < c["builds"] < c["chunks"]
    # neighbours mode: two words per wave and chunk, less what the guards w0 < nw and w0 + 1 < nw hold back
    assert c["word_stores"] + c["words_guarded"] == 4 * c["chunks"] and c["words_guarded"] > 1000


def test_bad_calls_are_refused_before_the_device_is_asked():
    """Every refusal of a clusters call is host code alone (smx_pairs_plan.h), for both entry points: on a machine
    without a GPU the same call with good jobs is the one that fails, with SMX_ERR_DEVICE.  A refused call leaves
    kernel_ms alone."""
    import numpy as np
    import torch
    from specimux_amd import _lib, calls
    lib = _lib.load()
    good = [b"ACGTACGT", b"ACGAACGT", b"", b"ACGT", b"ACGTT"]
    wide = bytes(range(256)) * 19 + bytes(64)          # 4928 bytes, 77 words x 256 distinct bytes: more than the LDS holds

    def call(neighbours, reads, jobs, roff=None):
        roff = calls.offsets(reads) if roff is None else np.array(roff, dtype=np.uint64)
        ks = np.full(len(reads), 3, dtype=np.int32)
        jarr = np.array(jobs, dtype=_lib.PAIRS_JOB_DTYPE)
        out = np.zeros(64, dtype=np.uint32)
        ms = _lib.C.c_float(-1.0)
        fn = lib.smx_pairs_neighbours if neighbours else lib.smx_pairs_distances
        rc = fn(b"".join(reads), _lib.ptr(roff), len(reads), _lib.ptr(ks), _lib.ptr(jarr), len(jobs), _lib.ptr(out), _lib.C.byref(ms))
        return rc, lib.smx_last_error().decode(), ms.value
    for neighbours in (False, True):
        for reads, jobs, roff, code, word in (
                (good, [(0, 5)], [0, 8, 16, 12, 20, 25], _lib.ERR_ARG, "query 2 is empty"),      # offsets that step back
                (good, [(3, 3)], None, _lib.ERR_ARG, "read range out of bounds"),
                (good, [(0, 3), (2, 3)], None, _lib.ERR_ARG, "jobs 0 and 1 overlap"),
                (good + [wide], [(0, 2)], None, _lib.ERR_UNSUPPORTED, "do not fit the LDS")):
            rc, msg, ms = call(neighbours, reads, jobs, roff)
            assert rc == code and word in msg and ms == -1.0, (neighbours, jobs, rc, msg, ms)
        # an empty read among the rows, a job of one read and a job of none: good
        rc, msg, ms = call(neighbours, good, [(0, 3), (3, 1), (4, 0), (4, 1)])
        if torch.cuda.is_available():
            assert rc == _lib.OK and ms >= 0.0, (rc, msg, ms)
        else:
            assert rc == _lib.ERR_DEVICE and ms == -1.0, (rc, msg, ms)
