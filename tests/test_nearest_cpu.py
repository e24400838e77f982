"""CPU simulation of the crosstalk call (specimux_amd/csrc/smx_nearest.hip): the host plan (smx_nearest_plan.h) and the
kernel as a host loop over the planned chunks (tests/cpu/nearest_host.h, which calls pairs_pair and smx_nearest_core.h as
the kernel does), against a plain O(mn) DP reduced by a two-line reference -- refs of every state class and the generic
one, 1 / 127 / 128 / 129 / 257 reads per job, runs of one ref, of the whole class and in between, two jobs sharing
refs, identical refs in one group and in two, reads within limit of no ref, empty reads, limits at d - 1, d, d + 1.  A
sample of the simulation's DP results is checked against the suite's oracle, and the counters it prints are bounded from
below so that its coverage cannot shrink unnoticed.  No GPU needed."""
import os
import subprocess

import pytest

from oracle.edlib_semantics import NW, align_c

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("nearest") / "nearest_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "tests", "cpu"), "-o", exe,
                           os.path.join(REPO, "tests", "cpu", "nearest_sim.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_nearest_plan_and_chunk_loop(sim, tmp_path, seed):
    out = subprocess.run([sim, str(seed)], capture_output=True, text=True, cwd=tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    c = {}
    for line in out.stdout.splitlines():
        key, _, val = line.partition(" ")
        if val.lstrip("-").isdigit() and key.isidentifier():
            c[key] = int(val)
    assert c["scenario_classes"] == 1 and c["scenario_reads"] == 1 and c["plans"] == 10
    # every state class: refs of 1 and 63-64 (1 word), 65-128 (2), 129-200 (4), 300-500 (8), 700-1024 (16), 1025-1100 (generic)
    for wr in (0, 1, 2, 4, 8, 16):
        assert c[f"class_{wr}"] >= 1000, wr
    # the run length: one ref, the whole class, in between -- as plans and as runs
    assert c["plans_run_len_1"] >= 2 and c["plans_run_len_class"] >= 2 and c["plans_run_len_between"] >= 2
    assert c["runs_of_one"] >= 100 and c["runs_of_class"] >= 40 and c["runs_between"] >= 20
    assert c["builds"] >= 500 and c["chunks"] >= 300 and c["pairs"] >= 40000 and c["dist_checked"] >= 8000
    # the tie rule within each key and across them; reads with both keys, one, none
    assert c["tie_within_own"] >= 40 and c["tie_within_other"] >= 30 and c["tie_across_keys"] >= 30
    for key in ("reads_both", "reads_own_only", "reads_other_only", "reads_no_key"):
        assert c[key] >= 80, key
    assert c["empty_reads"] >= 20
    for key in ("k_d_minus_1", "k_d", "k_d_plus_1"):
        assert c[key] >= 50, key
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
    assert n == c["oracle_sample"] >= 50


def test_bad_jobs_are_refused_before_the_device_is_asked():
    """An empty ref, an index out of range and overlapping read ranges are SMX_ERR_ARG from host code alone: on a machine
    without a GPU the same call with good jobs is the one that fails, with SMX_ERR_DEVICE."""
    import numpy as np
    import torch
    from specimux_amd import _lib, calls
    lib = _lib.load()
    seqs = [b"ACGTACGT", b"ACGAACGT", b"", b"ACGT", b"ACGTT"]
    off = calls.offsets(seqs)
    ks = np.array([2] * len(seqs), dtype=np.int32)
    group = np.arange(len(seqs), dtype=np.uint32)

    def call(jobs, nearest):
        jarr = np.array(jobs, dtype=_lib.NEAREST_JOB_DTYPE)
        a, b, d = np.zeros(64, dtype=np.uint64), np.zeros(64, dtype=np.uint64), np.zeros(64, dtype=np.int32)
        args = (b"".join(seqs), _lib.ptr(off), len(seqs), _lib.ptr(ks), _lib.ptr(group), _lib.ptr(jarr), len(jobs))
        rc = lib.smx_nearest(*args, _lib.ptr(a), _lib.ptr(b), None) if nearest else lib.smx_nearest_distances(*args, _lib.ptr(d), None)
        return rc, lib.smx_last_error().decode()
    for nearest in (True, False):
        rc, msg = call([(1, 2, 3, 2)], nearest)                          # sequence 2 is empty: as a ref
        assert rc == _lib.ERR_ARG and "empty ref" in msg
        rc, msg = call([(0, 2, 3, 3)], nearest)
        assert rc == _lib.ERR_ARG and "out of bounds" in msg
        rc, msg = call([(4, 2, 0, 1)], nearest)
        assert rc == _lib.ERR_ARG and "out of bounds" in msg
        rc, msg = call([(0, 2, 2, 2), (0, 1, 3, 2)], nearest)
        assert rc == _lib.ERR_ARG and "overlap" in msg
        # shared and overlapping refs, touching read ranges, an empty read, jobs without reads and without refs: good
        rc, msg = call([(0, 2, 2, 1), (0, 1, 3, 2), (0, 2, 0, 0), (3, 0, 0, 2)], nearest)
        assert rc == (_lib.OK if torch.cuda.is_available() else _lib.ERR_DEVICE), msg
