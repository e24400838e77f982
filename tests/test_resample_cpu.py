"""CPU simulation of the resampling kernel (specimux_amd/csrc/smx_resample.hip): its body as a host loop
(tests/cpu/resample_host.h) over the host/device core smx_resample_core.h and the plans of smx_cons_plan.h, against plain
loops over every replicate's 26-word vote table.  The counters the simulation prints are bounded from below so that its
coverage cannot shrink unnoticed.  The rule itself is checked against consensus.call_consensus as it stands, through the
plain-Python twin.  And the arguments smx_cons_resample refuses are refused by host code alone.  No GPU needed."""
import os
import random
import subprocess

import numpy as np
import pytest

from clusters_utils import mutate, rand_seq
from specimux_amd import consensus
from support_utils import job_rows, replicate_table, resample_reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("resample") / "resample_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", exe, os.path.join(REPO, "tests", "cpu", "resample_sim.cpp")])
    return exe


def run(sim, *args):
    out = subprocess.run([sim, *args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    counts = {}
    for line in out.stdout.splitlines():
        key, _, val = line.partition(" ")
        if val.lstrip("-").isdigit() and key.isidentifier():
            counts[key] = int(val)
    return counts


def cases_of(n_b):
    """The (a[4], del, ins) a replicate of n_b voters can have: five counts whose sum is at most n_b, and ins <= n_b."""
    from math import comb
    return comb(n_b + 5, 5) * (n_b + 1)


def test_keeps_rule_exhaustive(sim):
    c = run(sim, "exhaustive")
    assert c["cases"] == sum(cases_of(n) for n in range(7)) * 5 * 2 and c["last_cases"] * 2 == c["cases"]
    assert c["kept"] > 15000 and c["not_kept"] > 30000
    assert c["draft_wins_tie"] > 3000 and c["tie_without_draft"] > 3500
    assert c["half_deletions"] > 1500 and c["half_insertions"] > 3000 and c["last_half_insertions"] > 3000
    assert c["top_zero"] >= 700 and c["other_draft"] * 10 == c["cases"] and c["other_draft_kept"] > 40


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_resample_jobs_against_plain_loops(sim, seed):
    c = run(sim, "random", str(seed))
    assert c["calls"] == 12 and c["jobs"] >= 45 and c["jobs_without_members"] >= 5
    assert c["bits"] >= 1500000 and c["bits_clear"] >= 20000 and c["replicates_all_kept"] >= 5000
    assert c["clear_at_0"] >= 3000 and c["clear_at_m_minus_1"] >= 3000 and c["clear_at_m"] >= 100
    assert c["clear_on_other_draft"] >= 500 and c["members_above_limit"] >= 200 and c["empty_replicates"] >= 3000


# ------------------------------------------------------------------------------------------------ the rule, in Python
@pytest.fixture(scope="module")
def twin():
    """One job of the twin: a 60-nt draft with an `N`, 24 members -- ten carry another base at p = 0 and p = 59, fourteen an
    extra base behind the last one, five have a base less in a run, one is an unrelated read above its limit -- under four
    levels of random masks of different density."""
    rng = random.Random(91)
    q = list(rand_seq(rng, 60))
    q[30] = "N"
    q[20:24] = "GGGG"
    q = "".join(q)
    other = ("C" if q[0] != "C" else "A") + q[1:59] + ("C" if q[59] != "C" else "A")
    members = []
    for i in range(24):
        r = other if i < 10 else q
        if 6 <= i < 20:
            r = r + ("T" if q[59] != "T" else "G")
        if 18 <= i < 23:
            r = r[:20] + r[21:]
        if i % 4 == 3:
            r = mutate(rng, r, 0.04)
        members.append(r.replace("N", "A") if i % 2 else r)
    members[23] = rand_seq(rng, 60)
    reads = [r.encode() for r in members] + [q.encode()]
    ks, jobs = [8] * 25, [(24, 0, 24)]
    masks = np.array([[rng.getrandbits(64) & rng.getrandbits(64) if l % 2 else rng.getrandbits(64) | (rng.getrandbits(64) * (l // 2))
                       for _ in range(24)] for l in range(4)], dtype=np.uint64)
    dists, rows = job_rows(reads, ks, jobs[0])
    return q, reads, ks, jobs, masks, dists, rows, resample_reference(reads, ks, jobs, masks)[0]


def test_a_set_bit_is_a_column_call_consensus_leaves_alone(twin):
    """call_consensus over one column of a replicate's table -- the draft D[p] alone, the column's row and a zero row for
    the position behind it -- returns D[p] iff the replicate's bit of the column is set."""
    q, _reads, _ks, _jobs, masks, dists, rows, js = twin
    assert dists[23] == -1 and min(dists[:23]) >= 0
    rng = random.Random(92)
    seen = {True: 0, False: 0}
    pairs = [(l, b, p) for l in range(4) for b in rng.sample(range(64), 6) for p in rng.sample(range(60), 12)]
    pairs += [(l, b, p) for l in range(4) for b in range(0, 64, 7) for p in (0, 20, 30, 59)]
    assert len(pairs) > 400
    for l, b, p in pairs:
        table, n_b = replicate_table(rows, dists, masks[l], b)
        assert n_b == int(js.sub_aligned[l, b])
        column = np.vstack([table[p], np.zeros(26, dtype=np.uint32)])
        same = consensus.call_consensus(q[p], column, n_b) == q[p]
        assert same == bool((int(js.agree[l, p]) >> b) & 1), (l, b, p)
        seen[same] += 1
    assert seen[True] > 200 and seen[False] > 20


def test_the_last_word_is_the_insertion_test_alone(twin):
    """p = m with an empty draft: call_consensus returns "" iff the bit is set."""
    _q, _reads, _ks, _jobs, masks, dists, rows, js = twin
    seen = {True: 0, False: 0}
    for l in range(4):
        for b in range(64):
            table, n_b = replicate_table(rows, dists, masks[l], b)
            same = consensus.call_consensus("", table[60:61], n_b) == ""
            assert same == bool((int(js.agree[l, 60]) >> b) & 1), (l, b)
            seen[same] += 1
    assert seen[True] > 50 and seen[False] > 20


def test_all_columns_kept_means_the_sequence_is_reproduced(twin):
    """A replicate that keeps every column calls the draft itself.  (The converse does not hold: dropping one base of a
    run and inserting it next door yields the same string.)"""
    q, reads, ks, jobs, _masks, dists, rows, _js = twin
    # the draft here is not what the members call; take what they do call, and resample around that
    table, n = replicate_table(rows, dists, [2**64 - 1] * 24, 0)
    called = consensus.call_consensus(q, table, n)
    reads2 = reads[:24] + [called.encode()]
    rng = random.Random(93)
    masks = np.array([[rng.getrandbits(64) | rng.getrandbits(64) for _ in range(24)] for _ in range(3)], dtype=np.uint64)
    js = resample_reference(reads2, ks, jobs, masks)[0]
    dists2, rows2 = job_rows(reads2, ks, jobs[0])
    whole = 0
    for l in range(3):
        for b in range(64):
            if all((int(w) >> b) & 1 for w in js.agree[l]):
                whole += 1
                t, n_b = replicate_table(rows2, dists2, masks[l], b)
                assert consensus.call_consensus(called, t, n_b) == called, (l, b)
    assert whole > 20


# ------------------------------------------------------------------------------------------------ the refusals
def test_bad_resample_arguments_are_refused_before_the_device_is_asked():
    """n_levels of 0 or above 16 and a null masks beside members are SMX_ERR_ARG from host code alone, also where there is
    no job: on a machine without a GPU the same call with good arguments is the one that fails, with SMX_ERR_DEVICE.  The
    checks of the jobs come with the plan, as for smx_cons_votes."""
    import torch
    from specimux_amd import _lib, calls
    lib = _lib.load()
    reads = [b"ACGTACGT", b"ACGAACGT", b"", b"ACGT", b"ACGTT"]
    roff = calls.offsets(reads)
    ks = np.array([2] * len(reads), dtype=np.int32)

    def call(jobs, n_levels, with_masks=True):
        jarr = np.array(jobs, dtype=_lib.CONS_JOB_DTYPE)
        votes, aligned = np.zeros(4096, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
        masks = np.full(16 * 8, 2**64 - 1, dtype=np.uint64)
        agree, sub = np.zeros(16 * 64, dtype=np.uint64), np.zeros(8 * 16 * 64, dtype=np.uint32)
        rc = lib.smx_cons_resample(b"".join(reads), _lib.ptr(roff), len(reads), _lib.ptr(ks), _lib.ptr(jarr), len(jobs),
                                   _lib.ptr(masks) if with_masks else None, n_levels, _lib.ptr(votes), _lib.ptr(aligned),
                                   _lib.ptr(agree), _lib.ptr(sub), None)
        return rc, lib.smx_last_error().decode()
    good = [(0, 0, 2), (3, 2, 0), (0, 2, 3)]
    for jobs in (good, []):                                    # refused even where there is nothing to do
        for n_levels in (0, 17, 2**32 - 1):
            rc, msg = call(jobs, n_levels)
            assert rc == _lib.ERR_ARG and "n_levels" in msg, (n_levels, msg)
    rc, msg = call(good, 4, with_masks=False)
    assert rc == _lib.ERR_ARG and "masks" in msg
    rc, msg = call([(2, 0, 2)], 4)
    assert rc == _lib.ERR_ARG and "empty draft" in msg
    rc, msg = call([(0, 0, 3), (3, 2, 2)], 4)
    assert rc == _lib.ERR_ARG and "overlap" in msg
    for n_levels in (1, 16):
        rc, msg = call(good, n_levels)
        assert rc == (_lib.OK if torch.cuda.is_available() else _lib.ERR_DEVICE), msg
    assert call([], 1)[0] == _lib.OK and call([], 16, with_masks=False)[0] == _lib.OK
    # a null masks is no fault where no job has members: the device is asked, and nothing is read
    rc, msg = call([(3, 2, 0)], 2, with_masks=False)
    assert rc == (_lib.OK if torch.cuda.is_available() else _lib.ERR_DEVICE), msg
