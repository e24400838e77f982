"""CPU simulation of the identify call (specimux_amd/csrc/smx_hits.hip): the host plan (smx_hits_plan.h) and the kernel as
a host loop over the planned chunks (tests/cpu/hits_host.h, which calls mine_pair and smx_hits_core.h as the kernel does),
against a plain O(mn) HW DP under the pair rule reduced by a full sort -- patterns of every state class and the generic
one, windows of 1 / 127 / 128 / 129 / 257 texts on both sides, queries all shorter, all longer and mixed, an equal-length
pair whose two directions differ, coverage at the threshold and one byte short, a window that coverage empties, limits at
d - 1, d, d + 1 and none, K = 1, 3 and 16 with fewer, exactly and many more hits, identical targets, jobs sharing
targets, hits_insert in shuffled orders, the plan's refusals from lengths alone.  A sample of the simulation's DP results
is checked against the suite's oracle, and the counters it prints are bounded from below so that its coverage cannot
shrink unnoticed.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

from oracle.edlib_semantics import HW, align_c

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("hits") / "hits_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "tests", "cpu"), "-o", exe,
                           os.path.join(REPO, "tests", "cpu", "hits_sim.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_hits_plan_and_chunk_loop(sim, tmp_path, seed):
    out = subprocess.run([sim, str(seed)], capture_output=True, text=True, cwd=tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    c = {}
    for line in out.stdout.splitlines():
        key, _, val = line.partition(" ")
        if val.lstrip("-").isdigit() and key.isidentifier():
            c[key] = int(val)
    for name in ("mixed", "shorter", "longer", "windows", "coverage"):
        assert c[f"scenario_{name}"] == 1, name
    assert c["plans"] == 15                        # five scenarios x K = 1, 3, 16
    # every state class: patterns of 1 and 63-64 (1 word), 65-128 (2), 129-200 (4), 300-500 (8), 700-1024 (16), 1025-1100 (generic)
    for wr in (0, 1, 2, 4, 8, 16):
        assert c[f"class_{wr}"] >= 150, wr
    # both sides, and windows of every size around the chunk on each
    assert c["side_q_pairs"] >= 4000 and c["side_t_pairs"] >= 3000
    assert c["pairs_pattern_query"] >= 1500 and c["pairs_pattern_target"] >= 1000
    for side in "qt":
        for n in (1, 127, 128, 129, 257):
            assert c[f"window_{side}_{n}"] >= 1, (side, n)
    assert c["chunks"] >= 500 and c["builds"] >= 500 and c["pairs"] >= 8000 and c["dist_checked"] >= 10000
    # the tie rule at equal length, coverage at and just below the threshold, a window that coverage empties
    assert c["equal_length_pairs"] >= 20 and c["tie_rule_pinned"] >= 3
    assert c["cov_at_threshold"] >= 2 and c["cov_one_short"] >= 2 and c["cov_excluded"] >= 200 and c["windows_emptied"] >= 3
    for key in ("k_d_minus_1", "k_d", "k_d_plus_1", "k_negative"):
        assert c[key] >= 40, key
    # fewer than K, exactly K, many more than K hits; ties that the target index decides; the pre-check at work
    assert c["hits_fewer_than_K"] >= 500 and c["hits_exactly_K"] >= 30 and c["hits_many_more_than_K"] >= 20
    assert c["ties_to_lower_index"] >= 30
    assert c["inserts"] >= 2000 and c["atomics"] >= c["inserts"] - c["prechecked"] and c["prechecked"] >= 500
    assert c["shuffled_rows"] >= 3 * 1500
    assert c["refusals_checked"] == 17
    # the simulation's reference DP against the suite's oracle
    n = 0
    with open(tmp_path / "oracle_sample.txt") as fh:
        for line in fh:
            qh, th, k, want = line.split()
            q = bytes.fromhex(qh).decode("latin-1")
            t = bytes.fromhex(th).decode("latin-1")
            got = align_c(q, t, HW, int(k), iupac=False)["editDistance"]
            assert got == int(want), (len(q), len(t), k, want, got)
            n += 1
    assert n == c["oracle_sample"] >= 200


def test_bad_calls_are_refused_before_the_device_is_asked():
    """Every refusal is host code alone: on a machine without a GPU the same call with good arguments is the one that
    fails, with SMX_ERR_DEVICE."""
    import torch
    from specimux_amd import _lib, calls
    lib = _lib.load()
    seqs = [b"ACGTACGT", b"ACGAACGT", b"", b"ACGT", b"ACGTT"]
    off = calls.offsets(seqs)
    ks = np.array([2] * len(seqs), dtype=np.int32)

    def call(jobs, hits, K=5, cov=500):
        jarr = np.array(jobs, dtype=_lib.HITS_JOB_DTYPE)
        a, d = np.zeros(256, dtype=np.uint64), np.zeros(64, dtype=np.int32)
        args = (b"".join(seqs), _lib.ptr(off), len(seqs), _lib.ptr(ks), _lib.ptr(jarr), len(jobs), K, cov)
        rc = lib.smx_best_hits(*args, _lib.ptr(a), None) if hits else lib.smx_best_hits_distances(*args, _lib.ptr(d), None)
        return rc, lib.smx_last_error().decode()
    for hits in (True, False):
        for jobs, kw, word in (([(1, 2, 3, 2)], {}, "empty"), ([(0, 2, 2, 2)], {}, "empty"), ([(0, 2, 3, 3)], {}, "out of bounds"),
                               ([(4, 2, 0, 1)], {}, "out of bounds"), ([(0, 2, 3, 1), (1, 1, 4, 1)], {}, "overlap"),
                               ([(0, 2, 3, 2)], {"K": 0}, "K = 0"), ([(0, 2, 3, 2)], {"K": 17}, "K = 17"),
                               ([(0, 2, 3, 2)], {"cov": 1001}, "min_cov_permille")):
            rc, msg = call(jobs, hits, **kw)
            assert rc == _lib.ERR_ARG and word in msg, (jobs, kw, rc, msg)
        # shared targets, jobs without queries and without targets: good
        rc, msg = call([(0, 1, 3, 2), (1, 1, 3, 2), (0, 0, 3, 2), (4, 1, 0, 0)], hits)
        assert rc == (_lib.OK if torch.cuda.is_available() else _lib.ERR_DEVICE), msg


def test_a_job_of_more_than_2_24_targets_is_unsupported():
    from specimux_amd import _lib, calls
    lib = _lib.load()
    n = 2**24 + 2                                  # one query, 2^24 + 1 targets, one byte each
    off = np.arange(n + 1, dtype=np.uint64)
    ks = np.zeros(n, dtype=np.int32)
    jarr = np.array([(0, 1, 1, n - 1)], dtype=_lib.HITS_JOB_DTYPE)
    keys = np.zeros(16, dtype=np.uint64)
    rc = lib.smx_best_hits(b"A" * n, _lib.ptr(off), n, _lib.ptr(ks), _lib.ptr(jarr), 1, 5, 500, _lib.ptr(keys), None)
    assert rc == _lib.ERR_UNSUPPORTED and "2^24" in lib.smx_last_error().decode()
