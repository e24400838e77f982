"""CPU simulation of the bimera call (specimux_amd/csrc/smx_reach.hip): the host plan (smx_reach_plan.h) and the kernel as
a host loop over the planned chunks (tests/cpu/reach_host.h, which calls smx_reach_core.h as the kernel does), against the
plain O(nm) DP of the definition reduced by a full sort -- lengths 1, 7, 8, 9, 15, 16, 17, 63, 64, 65 on both sides,
queries longer and shorter than the target, a target that is a proper prefix of the query, identical and unrelated pairs,
E = 0, 1, 5, 15, a first mismatch at byte 7 / 8 / 9 of a slide, a match to the end of the shorter sequence with equal
bytes behind it, slides from every offset mod 8, both sides, eligibility at weight = need and need - 1 and t = q, identical
targets, 0 / 1 / 2 / 3 eligible targets, jobs sharing targets and without queries or targets, 1 / 2 / 3 / 63 / 64 / 65
pairs per job, hits_insert in shuffled orders, the plan's refusals from lengths alone.  The counters it prints are bounded
from below so that its coverage cannot shrink unnoticed.  The Python twin of the tests (tests/bimera_utils.py) is checked
against a third, plainest DP here.  No GPU needed."""
import os
import random
import subprocess

import numpy as np
import pytest

import bimera_utils as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("reach") / "reach_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "tests", "cpu"), "-o", exe,
                           os.path.join(REPO, "tests", "cpu", "reach_sim.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reach_plan_and_chunk_loop(sim, tmp_path, seed):
    out = subprocess.run([sim, str(seed)], capture_output=True, text=True, cwd=tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    c = {}
    for line in out.stdout.splitlines():
        key, _, val = line.partition(" ")
        if val.lstrip("-").isdigit() and key.isidentifier():
            c[key] = int(val)
    for name in ("lengths", "padding", "eligibility", "shapes", "random"):
        assert c[f"scenario_{name}"] == 1, name
    assert c["plans"] == 20                        # five scenarios x E = 0, 1, 5, 15
    assert c["values_checked"] >= 500000 and c["keys_checked"] >= 15000 and c["items"] >= 80000 and c["chunks"] >= 1000
    assert c["side_left"] == c["side_right"] >= 40000
    for g in range(4):
        assert c[f"group_{g}"] >= 15000, g
    # the pairs the slide and the clamps can go wrong on
    assert c["query_longer"] >= 3000 and c["query_shorter"] >= 3000 and c["identical_pairs"] >= 30
    assert c["target_proper_prefix"] >= 300 and c["unrelated_pairs"] >= 2000 and c["length_one"] >= 500
    for at in (7, 8, 9):
        assert c[f"first_mismatch_at_{at}"] >= 100, at
    assert c["first_mismatch_at_15_17"] >= 100
    assert c["equal_beyond_the_end"] >= 50 and c["equal_beyond_the_end_next_sequence"] >= 20
    for x in range(8):
        assert c[f"slide_q_mod8_{x}"] >= 100000 and c[f"slide_r_mod8_{x}"] >= 100000, x
        assert c[f"offset_mod8_{x}"] >= 20, x
    assert c["steps"] >= 100000 and c["slides"] >= 1000000 and c["early_ends"] >= 5000
    # eligibility, the sizes of jobs, the reduction
    assert c["weight_at_need"] >= 3 and c["weight_one_short"] >= 3 and c["target_is_query"] >= 100 and c["not_eligible"] >= 500
    for n in (0, 1, 2, 3):
        assert c[f"eligible_{n}"] >= 1, n
    for n in (1, 2, 3, 63, 64, 65):
        assert c[f"job_pairs_{n}"] >= 1, n
    assert c["jobs_without_queries"] >= 1 and c["jobs_without_targets"] >= 1
    assert c["ties_to_lower_index"] >= 2000
    assert c["inserts"] >= 300000 and c["atomics"] >= c["inserts"] - c["prechecked"] and c["prechecked"] >= 100000
    assert c["shuffled_slots"] >= 3 * 5000
    assert c["refusals_checked"] == 15


def plainest_reach(q: bytes, r: bytes, E: int):
    n, m = len(q), len(r)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
            else:
                D[i][j] = min(D[i - 1][j - 1] + (q[i - 1] != r[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return [max(i for i in range(n + 1) if min(D[i]) <= e) for e in range(E + 1)]


def test_the_twin_is_the_definition():
    rng = random.Random(4)
    for _ in range(300):
        q = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(1, 30)))
        kind = rng.randrange(3)
        r = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(1, 30))) if kind == 0 else \
            q[:rng.randrange(1, len(q) + 1)] if kind == 1 else \
            bytes(c if rng.random() > 0.15 else rng.choice(b"ACGT") for c in q) + b"GG"[:rng.randrange(3)]
        E = rng.choice((0, 1, 5, 15))
        assert U.reach_reference(q, r, E) == plainest_reach(q, r, E), (q, r, E)
    assert U.reach_reference(b"ACGTACGT", b"ACGT", 3) == [4, 5, 6, 7]      # a proper prefix: one byte per further edit
    assert U.reach_reference(b"ACGT", b"ACGTTTTT", 0) == [4]
    assert U.reach_reference(b"AAAA", b"CCCC", 2) == [0, 1, 2]


def test_bad_calls_are_refused_before_the_device_is_asked():
    """Every refusal is host code alone: on a machine without a GPU the same call with good arguments is the one that
    fails, with SMX_ERR_DEVICE."""
    import torch
    from specimux_amd import _lib, calls
    lib = _lib.load()
    seqs = [b"ACGTACGT", b"ACGAACGT", b"", b"ACGT", b"ACGTT"]
    off = calls.offsets(seqs)
    w = np.array([1] * len(seqs), dtype=np.uint32)

    def call(jobs, keys, E=5, off=off):
        jarr = np.array(jobs, dtype=_lib.REACH_JOB_DTYPE)
        a, v = np.zeros(1024, dtype=np.uint64), np.zeros(1024, dtype=np.uint32)
        args = (b"".join(seqs), _lib.ptr(off), len(seqs), _lib.ptr(w), _lib.ptr(w), _lib.ptr(jarr), len(jobs), E)
        rc = lib.smx_prefix_reach(*args, _lib.ptr(a), None) if keys else lib.smx_prefix_reach_matrix(*args, _lib.ptr(v), None)
        return rc, lib.smx_last_error().decode()
    fall = off.copy()
    fall[2] = 4
    for keys in (True, False):
        for jobs, kw, word in (([(1, 2, 3, 2)], {}, "empty"), ([(0, 2, 2, 2)], {}, "empty"), ([(0, 2, 3, 3)], {}, "out of bounds"),
                               ([(4, 2, 0, 1)], {}, "out of bounds"), ([(0, 2, 3, 1), (1, 1, 4, 1)], {}, "overlap"),
                               ([(0, 2, 3, 2)], {"E": 16}, "E = 16"), ([(0, 2, 3, 2)], {"off": fall}, "bad offsets")):
            rc, msg = call(jobs, keys, **kw)
            assert rc == _lib.ERR_ARG and word in msg, (jobs, kw, rc, msg)
        # shared targets, queries that are targets, jobs without queries and without targets: good
        rc, msg = call([(0, 1, 3, 2), (1, 1, 3, 2), (0, 0, 3, 2), (4, 1, 0, 0), (3, 1, 0, 2)], keys)
        assert rc == (_lib.OK if torch.cuda.is_available() else _lib.ERR_DEVICE), msg
    assert _lib.ABI_VERSION == 13 and lib.smx_abi_version() == 13
