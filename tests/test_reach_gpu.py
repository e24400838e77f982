"""The bimera kernel on the GPU (smx_reach.hip): smx_prefix_reach_matrix and smx_prefix_reach against the plain-Python twin
(tests/bimera_utils.py: the O(nm) DP of the definition, a full sort) on 70 sequences of at most 130 nt -- lengths 1, 7, 8,
9, 15, 16, 17, 63, 64, 65 on both sides, prefixes and suffixes of one another, a first mismatch at byte 7 / 8 / 9 from
either end, twins, strangers, every sequence a query and a target, weights at need and need - 1, jobs of 1, 2, 3, 63, 64
and 65 pairs over shared targets, jobs without queries and without targets; E = 0, 1, 5 and 15; two calls give the same
bytes; a small call after a large one; refusals launch nothing and say why; a parent pool cut into three pieces gives the
one-piece result."""
import random

import numpy as np
import pytest

import bimera_utils as U
from specimux_amd import _lib, bimera, calls, identify

pytestmark = pytest.mark.gpu

LENGTHS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65)


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def edit(rng, s, k):
    out = list(s)
    for _ in range(k):
        p = rng.randrange(len(out))
        kind = rng.randrange(3)
        if kind == 0:
            out[p] = "A" if out[p] != "A" else "C"
        elif kind == 1:
            out.insert(p, rng.choice("ACGT"))
        elif len(out) > 1:
            del out[p]
    return "".join(out)


def flip(s, at):
    return s[:at] + ("G" if s[at] != "G" else "T") + s[at + 1:] if at < len(s) else s


def build_case(seed=7):
    rng = random.Random(seed)
    a, b = rand_seq(rng, 130), rand_seq(rng, 130)
    seqs = []
    for i, L in enumerate(LENGTHS):
        fa, fb = a[:L], b[130 - L:]
        at = (7, 8, 9)[i % 3]
        seqs += [fa, fb, edit(rng, fa, 1 + i % 3), flip(fa, at), flip(fb[::-1], at)[::-1], rand_seq(rng, L)]
    seqs += [a, a[:100], seqs[0]]                  # the longest; a proper prefix of it; a twin of the first
    family = len(seqs)
    assert family == 63
    seqs += [edit(rng, a[:40], i % 3) for i in range(7)]
    weights = [1 + i % 4 for i in range(len(seqs))]
    needs = [i % 5 for i in range(family)] + [2] * 7
    jobs = [(0, family, 0, family)]
    for i, nt in enumerate((1, 2, 3, 63, 64, 65)):
        jobs.append((family + i, 1, 0, nt))        # shared targets; the last one's include another job's query
    jobs.append((0, 0, 3, 9))                      # no queries
    jobs.append((family + 6, 1, 0, 0))             # no targets: its rows stay empty
    assert len(seqs) == 70 and max(len(s) for s in seqs) == 130
    return [s.encode("latin-1") for s in seqs], weights, needs, jobs


@pytest.fixture(scope="module")
def case():
    seqs, weights, needs, jobs = build_case()
    want = U.matrix_reference(seqs, weights, needs, jobs, bimera.MAX_E)        # once, at E = 15: reach(e) does not depend on E
    m = want[0]
    elig = m[:, :, 0, 0] != bimera.NOT_ELIGIBLE
    assert elig.sum() >= 1500 and (~elig).sum() >= 1000 and not elig.diagonal().any()
    assert sum(1 for q in range(63) for t in range(63) if weights[t] == needs[q]) >= 300
    assert sum(1 for q in range(63) for t in range(63) if weights[t] + 1 == needs[q]) >= 300
    lens = np.array([len(s) for s in seqs[:63]])
    full = (m[:, :, 0, 15] == lens[:, None]) & elig
    assert (full & (m[:, :, 0, 0] != lens[:, None])).sum() >= 100              # reached only with edits
    assert ((m[:, :, 0, 15] < lens[:, None]) & elig).sum() >= 300              # never reached
    assert ((m[:, :, 1, 0] == lens[:, None]) & elig).sum() >= 20               # the right side at no edits
    return seqs, weights, needs, jobs, want


@pytest.mark.parametrize("E", [0, 1, 5, 15])
def test_matrix_matches_the_twin(case, E):
    seqs, weights, needs, jobs, want = case
    got = bimera.reach_matrix(seqs, weights, needs, jobs, E)
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        w = w[:, :, :, :E + 1]
        assert g.shape == w.shape and not (g == 0x5A5A5A5A).any(), j
        bad = np.argwhere(g != w)
        assert bad.size == 0, (j, jobs[j], bad[:5].tolist(), [(int(g[tuple(x)]), int(w[tuple(x)])) for x in bad[:5]])


@pytest.mark.parametrize("E", [0, 1, 5, 15])
def test_keys_equal_the_sorted_reference(case, E):
    seqs, weights, needs, jobs, _ = case
    keys = bimera.reach(seqs, weights, needs, jobs, E)
    ref = U.keys_reference(seqs, weights, needs, jobs, E)
    assert keys.shape == ref.shape and (keys == ref).all(), np.argwhere(keys != ref)[:5].tolist()
    pairs = keys.reshape(-1, bimera.SLOTS)
    filled = (pairs != np.uint64(bimera.NONE)).sum(axis=1)
    assert (filled == 0).sum() >= 2 * (E + 1) and (filled == 1).sum() >= 2 * (E + 1) and (filled == 2).sum() >= 100
    again = bimera.reach(seqs, weights, needs, jobs, E)
    assert again.tobytes() == keys.tobytes()       # two calls give the same bytes


def test_a_small_call_after_a_large_one(case):
    seqs, weights, needs, jobs, _ = case
    bimera.reach(seqs, weights, needs, jobs, 15)   # grows the workspace
    small = [b"ACGTACGTAC", b"ACGTACGTACTT", b"ACGAACGTAC", b"GGGGGGGGGGGG", b"ACGTACGTAC"]
    keys = bimera.reach(small, [1] * 5, [0] * 5, [(0, 1, 1, 4)], 1).reshape(2, 2, 2)
    want_left = [[bimera.pack_key(10, 1), bimera.pack_key(10, 4)], [bimera.pack_key(10, 1), bimera.pack_key(10, 2)]]
    want_right = [[bimera.pack_key(10, 4), bimera.pack_key(6, 2)], [bimera.pack_key(10, 2), bimera.pack_key(10, 4)]]
    assert [[int(x) for x in row] for row in keys[0]] == want_left
    assert [[int(x) for x in row] for row in keys[1]] == want_right
    m = bimera.reach_matrix(small, [1] * 5, [0, 0, 0, 0, 2], [(0, 1, 1, 4), (4, 1, 0, 2)], 1)
    assert m[0][0, :, 0, :].tolist() == [[10, 10], [3, 10], [0, 1], [10, 10]]
    assert (m[1] == bimera.NOT_ELIGIBLE).all()     # need 2 > every weight


def test_refusals_launch_nothing():
    lib = _lib.load()
    seqs = [b"ACGTACGT", b"ACGAACGT", b"", b"ACGT", b"ACGTT"]
    off = calls.offsets(seqs)
    w = np.ones(len(seqs), dtype=np.uint32)

    def call(jobs, E=5, matrix=False):
        jarr = np.array(jobs, dtype=_lib.REACH_JOB_DTYPE)
        a = np.full(1024, 0x5A, dtype=np.uint64)
        ms = _lib.C.c_float(-1.0)                  # its own kernel_ms, and so a direct call: a refusal must leave it alone
        fn = lib.smx_prefix_reach_matrix if matrix else lib.smx_prefix_reach
        rc = fn(b"".join(seqs), _lib.ptr(off), len(seqs), _lib.ptr(w), _lib.ptr(w), _lib.ptr(jarr), len(jobs), E, _lib.ptr(a),
                _lib.C.byref(ms))
        return rc, lib.smx_last_error().decode(), a, ms.value
    for matrix in (False, True):
        for jobs, kw, word in (([(1, 2, 3, 2)], {}, "empty"), ([(0, 2, 2, 2)], {}, "empty"), ([(0, 6, 3, 1)], {}, "out of bounds"),
                               ([(0, 2, 3, 1), (1, 1, 4, 1)], {}, "overlap"), ([(0, 2, 3, 2)], {"E": 16}, "E = 16")):
            rc, msg, a, ms = call(jobs, matrix=matrix, **kw)
            assert rc == _lib.ERR_ARG and word in msg, (jobs, rc, msg)
            assert (a == 0x5A).all() and ms == -1.0    # neither the output nor the kernel time were touched
    rc, msg, a, ms = call([(0, 1, 3, 2), (1, 1, 3, 2)], E=0)                   # shared targets
    assert rc == _lib.OK and ms >= 0.0, msg
    want = U.keys_reference(seqs, [1] * 5, [1] * 5, [(0, 1, 3, 2), (1, 1, 3, 2)], 0)
    assert (a[:want.size] == want).all() and int(want[0]) == bimera.pack_key(4, 3)


def test_three_pieces_of_a_pool_give_the_one_piece_result(case):
    seqs = [s.decode("latin-1") for s in case[0]]
    called = [bimera.Called(f"S{i // 3}_c{i % 3 + 1}", f"S{i // 3}", (40, 9, 3)[i % 3], f"S{i // 3}_c{i % 3 + 1}", seqs[i])
              for i in range(30, 48)]
    pool = [identify.Record(f"ref{i}", seqs[i]) for i in (60, 61, 36, 37, 42, 43, 12, 13, 18)]
    one, s1 = bimera.bimera(called, pool, "specimen", 2, 3, 2.0, budget=1 << 30)
    room = sum(len(c.seq) for c in called) + sum(len(p.seq) for p in pool) // 3 + 40
    three, s3 = bimera.bimera(called, pool, "specimen", 2, 3, 2.0, budget=room)
    assert s1["device_calls"] == 2 and s3["device_calls"] == 4
    assert [U.verdict_tuple(v) for v in three] == [U.verdict_tuple(v) for v in one]
    assert [U.verdict_tuple(v) for v in one] == U.verdicts_reference(called, pool, "specimen", 2, 3, 2.0)
    assert sum(v.left is not None and v.left >= len(called) for v in one) >= 3   # parents from the pool are named
