"""CPU simulation of whole specimine calls: the plan (specimux_amd/csrc/smx_mine_plan.h) and the kernel as a host loop over
the planned chunks (tests/cpu/mine_host.h, the first record of every workgroup found by chunk_owner's search over 64 emulated
lanes), every distance and best identity compared (==) with the full-matrix HW recurrence of tests/cpu/mine_plan_sim.cpp.
The counters the simulation prints are asserted, so that a shape that stops reaching a class, a second chunk or the capped
grid fails.  No GPU needed."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("mine_plan") / "mine_plan_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "tests", "cpu"), "-o", exe, os.path.join(REPO, "tests", "cpu", "mine_plan_sim.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    return {key: int(val) for key, _, val in (line.partition(" ") for line in out.stdout.splitlines()) if key.isidentifier()}


def test_every_output_equals_the_plain_dp(counts):
    c = counts
    # four limit variants (-1, 0, m / 10, above m, rotating over the queries) x the production budget and one slice
    assert c["plans"] == 8 and c["capped_plans"] == 4
    # jobs: 2 x (11 queries x 300 targets) + 3 x 1 + 3 x 127 + 3 x 128 + 3 x 129 + 2 x 2; a best identity per job target
    pairs = 2 * 11 * 300 + 3 * 1 + 3 * 127 + 3 * 128 + 3 * 129 + 2 * 2
    best = 2 * 300 + 1 + 127 + 128 + 129 + 10 + 2
    assert c["pairs"] == 8 * pairs and c["compared"] == 8 * (pairs + best)
    assert c["within"] > 30000 and c["beyond"] > 20000 and c["best_set"] > 4000
    assert c["ref_pairs"] > 3500


def test_the_shapes_reach_every_class_and_the_chunk_walk(counts):
    c = counts
    for cls in range(6):
        assert c[f"class_pairs_{cls}"] > 5000 and c[f"class_blocks_{cls}"] >= 8, cls
    # records of two and three chunks, workgroups that start inside a record, tables shared by the records of a query
    assert c["records"] == 8 * (2 * 11 + 4 * 3 + 2) and c["records_two_chunks"] >= 8 * 22
    assert c["blocks_inside"] >= 8 and c["builds"] < c["records"] < c["chunks"]
    # with a budget of one slice the generic class is one workgroup: 4 of the 8 plans have 2 blocks there, 4 have 1
    assert c["class_blocks_0"] == 4 * 2 + 4 * 1


def test_owner_search_takes_up_to_four_rounds(counts):
    # prefixes of 1 .. 300 001 records: the 64-lane search against std::upper_bound, a fourth round from 262 145 records on
    assert counts["owner_sweep_rounds"] == 4 and counts["owner_sweep_searches"] > 5000


def test_bad_calls_are_refused_before_the_device_is_asked():
    """Every refusal of a specimine call is host code alone (smx_mine_plan.h), for both entry points: on a machine
    without a GPU the same call with good jobs is the one that fails, with SMX_ERR_DEVICE.  A refused call leaves
    kernel_ms alone."""
    import numpy as np
    import torch
    from specimux_amd import _lib, calls
    lib = _lib.load()
    good_q, good_t = [b"ACGTACGT", b"ACGAACG"], [b"TTACGTACGTTT", b"ACGAACGT", b"GGGG"]
    wide = bytes(range(256)) * 19 + bytes(64)          # 4928 bytes, 77 words x 256 distinct bytes: more than the LDS holds

    def call(best, queries, targets, jobs, toff=None):
        qoff, toff = calls.offsets(queries), calls.offsets(targets) if toff is None else np.array(toff, dtype=np.uint64)
        ks = np.full(len(queries), 3, dtype=np.int32)
        jarr = np.array(jobs, dtype=_lib.MINE_JOB_DTYPE)
        out = np.zeros(64, dtype=np.float64 if best else np.int32)
        ms = _lib.C.c_float(-1.0)
        fn = lib.smx_mine_best_identity if best else lib.smx_mine_distances
        rc = fn(b"".join(queries), _lib.ptr(qoff), len(queries), _lib.ptr(ks), b"".join(targets), _lib.ptr(toff), len(targets),
                _lib.ptr(jarr), len(jobs), _lib.ptr(out), _lib.C.byref(ms))
        return rc, lib.smx_last_error().decode(), ms.value
    for best in (False, True):
        for queries, jobs, toff, code, word in (
                ([b"ACGT", b""], [(0, 1, 0, 3, 0.5)], None, _lib.ERR_ARG, "query 1 is empty"),
                (good_q, [(1, 2, 0, 3, 0.5)], None, _lib.ERR_ARG, "out of bounds"),
                (good_q, [(0, 2, 2, 2, 0.5)], None, _lib.ERR_ARG, "out of bounds"),
                (good_q, [(0, 2, 0, 3, 0.5)], [0, 12, 8, 24], _lib.ERR_ARG, "target 1: bad offsets"),
                ([b"ACGT", wide], [(0, 1, 0, 3, 0.5)], None, _lib.ERR_UNSUPPORTED, "do not fit the LDS")):
            rc, msg, ms = call(best, queries, good_t, jobs, toff)
            assert rc == code and word in msg and ms == -1.0, (best, jobs, rc, msg, ms)
        # a job without targets and one without queries next to a full one: good
        rc, msg, ms = call(best, good_q, good_t, [(0, 2, 0, 3, 0.5), (0, 1, 3, 0, 0.5), (2, 0, 0, 2, 0.5)])
        if torch.cuda.is_available():
            assert rc == _lib.OK and ms >= 0.0, (rc, msg, ms)
        else:
            assert rc == _lib.ERR_DEVICE and ms == -1.0, (rc, msg, ms)
