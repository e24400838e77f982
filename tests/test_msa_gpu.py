"""smx_msa on the GPU against its numpy twin (tests/msa_utils.py msa_reference), by == on the rows, the lengths and the
costs.  The shapes are the smallest at which each part of the merge kernel can go wrong: a direction word of 16 cells, a
band of 64 rows, a round of 16 bands (1 024 rows), the walk's tile of 64 rows x 256 columns, the build's chunks over 1 024
threads, the 64-bit scores, the level loop, the cutting of a level and the workspace's reuse."""
import functools

import numpy as np
import pytest

import msa_utils as U
from specimux_amd import _lib, calls

pytestmark = pytest.mark.gpu


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def tree_case(n: int, kind: str, seed: int = 0):
    """(seqs, merges) of n related sequences of 20-40 nt under a tree of `kind`, computed once per test run."""
    rng = np.random.default_rng(1000 * n + seed)
    root = U.random_seq(rng, 40)
    seqs = tuple(U.mutate(rng, root, 0.25)[:40].ljust(20, b"A") for _ in range(n))
    merges = {"random": lambda: U.random_tree(rng, n), "ladder": lambda: U.ladder_tree(n), "balanced": lambda: U.balanced_tree(n)}[kind]()
    return seqs, tuple(merges)


@functools.lru_cache(maxsize=None)
def twin(seqs, merges, X, G):
    return frozen(*U.msa_reference(seqs, merges, X, G))


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def check(seqs, merges, X=1, G=1):
    seqs, merges = tuple(seqs), tuple(merges)
    got = calls.msa(seqs, merges, X, G)
    want = twin(seqs, merges, X, G)
    assert same(got, want), (len(seqs), [len(s) for s in seqs][:4], X, G)
    return got


def degapped(rows):
    return [bytes(r[r != U.GAP].tolist()) for r in rows]


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 9])
def test_small_trees(n):
    seqs, merges = tree_case(n, "random")
    rows, lens, costs = check(seqs, merges)
    assert rows.shape[0] == n and len(lens) == len(costs) == max(n - 1, 0)
    assert degapped(rows) == list(seqs)


@functools.lru_cache(maxsize=None)
def pair_case(la: int, lb: int):
    rng = np.random.default_rng(la * 10007 + lb)
    a = U.random_seq(rng, la)
    b = U.random_seq(rng, lb) if min(la, lb) < 8 or max(la, lb) > 2 * min(la, lb) else (U.mutate(rng, a, 0.15) + U.random_seq(rng, lb))[:lb]
    return a, b


# (1, 1), (1, 300): the edges; 15 / 16 / 17 / 33: the direction word; 63 / 64 / 65 / 129: a band; 1 025: one row above the
# 16 x 64 rows the workgroup covers in a round; 2 100: a whole round above
@pytest.mark.parametrize("la, lb", [(1, 1), (1, 300), (300, 1), (15, 17), (16, 16), (17, 33), (63, 65), (64, 64), (65, 129),
                                    (300, 3), (1025, 1030), (2100, 2050)])
def test_pairs(la, lb):
    a, b = pair_case(la, lb)
    rows, lens, costs = check((a, b), ((0, 1),))
    assert degapped(rows) == [a, b]


def test_identical_sequences_are_all_diagonal():
    a = U.random_seq(np.random.default_rng(3), 333)
    rows, lens, costs = check((a, a), ((0, 1),))
    assert lens.tolist() == [333] and costs.tolist() == [0] and bytes(rows[0].tolist()) == bytes(rows[1].tolist()) == a


def test_a_deletion_of_40_bases():
    a = U.random_seq(np.random.default_rng(4), 400)
    b = a[:180] + a[220:]
    rows, lens, costs = check((a, b), ((0, 1),), 2, 3)
    assert lens.tolist() == [400] and costs.tolist() == [40 * 3]


def test_unrelated_sequences():
    rng = np.random.default_rng(5)
    check((U.random_seq(rng, 500), U.random_seq(rng, 470)), ((0, 1),), 5, 2)


@pytest.mark.parametrize("X, G", [(1, 1), (2, 3)])
def test_33_tips_on_a_ladder_and_on_a_balanced_tree(X, G):
    seqs, ladder = tree_case(33, "ladder")
    _, balanced = tree_case(33, "balanced")
    first, second = check(seqs, ladder, X, G), check(seqs, balanced, X, G)
    assert degapped(first[0]) == degapped(second[0]) == list(seqs)
    assert first[0].shape != second[0].shape or not np.array_equal(first[0], second[0])
    assert not (first[0] == U.GAP).all(axis=0).any() and not (second[0] == U.GAP).all(axis=0).any()


def test_every_path_is_optimal():
    """Sequences of one repeated base: every monotone path with the most diagonals costs the same, the rule picks one."""
    seqs = (b"A" * 70, b"A" * 45, b"A" * 130, b"A" * 17, b"A" * 64)
    rows, lens, costs = check(seqs, U.ladder_tree(5))
    assert rows.shape[1] == 130 and costs[0] == 25
    check(seqs, U.balanced_tree(5), 2, 3)


def two_groups(per_group: int):
    seqs = (b"A" * 100,) * per_group + (b"C" * 100,) * per_group
    n, merges = 2 * per_group, []
    inner = U.balanced_tree(per_group)                   # within a group, in the group's own numbering
    for g in range(2):
        base = len(merges)
        merges += [tuple(x + g * per_group if x < per_group else n + base + (x - per_group) for x in m) for m in inner]
    merges.append((n + per_group - 2, n + 2 * (per_group - 1) - 1))
    return seqs, tuple(merges)


def test_scores_above_32_bits():
    """600 tips, two groups of 300 identical sequences: the last merge costs 300 x 300 x 100 mismatches of weight 1000 =
    9 x 10^9, every other merge nothing.  The gap weighs 1000 as well: two gaps may not be cheaper than a mismatch."""
    seqs, merges = two_groups(300)
    rows, lens, costs = calls.msa(seqs, merges, 1000, 1000)
    assert costs[:-1].tolist() == [0] * 598 and int(costs[-1]) == 300 * 300 * 100 * 1000 > 2**32
    assert lens.tolist() == [100] * 599 and rows.shape == (600, 100)
    assert (rows[:300] == ord("A")).all() and (rows[300:] == ord("C")).all()
    check(*two_groups(20), 1000, 1000)


def test_overflow_reports_the_columns_and_leaves_the_rows():
    seqs, merges = tree_case(9, "random")
    want = twin(seqs, merges, 1, 1)
    n, cols = 9, want[0].shape[1]
    marr = np.array(list(merges), dtype=_lib.MSA_MERGE_DTYPE)

    def call(cap):
        rows = np.full(n * max(cap, 1), 0x5A, dtype=np.uint8)
        n_cols, lens, costs = np.zeros(1, np.uint32), np.zeros(n - 1, np.uint32), np.zeros(n - 1, np.uint64)
        rc = calls.invoke("smx_msa", b"".join(seqs), _lib.ptr(calls.offsets(seqs)), n, _lib.ptr(marr), 1, 1, cap, _lib.ptr(rows),
                          _lib.ptr(n_cols), _lib.ptr(lens), _lib.ptr(costs), check=False)
        return rc, rows, int(n_cols[0]), lens, costs
    rc, rows, n_cols, lens, costs = call(cols - 1)
    assert rc == _lib.ERR_OVERFLOW and n_cols == cols and (rows == 0x5A).all()
    assert np.array_equal(lens, want[1]) and np.array_equal(costs, want[2])
    rc, rows, n_cols, lens, costs = call(n_cols)
    assert rc == _lib.OK and np.array_equal(rows.reshape(n, cols), want[0])
    assert same(calls.msa(seqs, merges, cap_cols=cols - 1), want)          # the binding's one retry


def test_a_level_cut_into_launches(monkeypatch):
    seqs, merges = tree_case(33, "balanced")
    whole = check(seqs, merges, 2, 3)
    monkeypatch.setenv("SMX_CLUSTERS_BUDGET_BYTES", "1")                    # one merge a launch
    assert same(calls.msa(seqs, merges, 2, 3), whole)
    monkeypatch.setenv("SMX_CLUSTERS_BUDGET_BYTES", "3000")                 # a few
    assert same(calls.msa(seqs, merges, 2, 3), whole)


def test_no_stale_workspace_and_the_same_call_twice():
    a, b = pair_case(1025, 1030)
    check((a, b), ((0, 1),))
    seqs, merges = tree_case(9, "random")
    after = check(seqs, merges)
    alone = check(seqs, merges)
    assert same(after, alone)
    ms = []
    first, second = calls.msa(seqs, merges, kernel_ms=ms), calls.msa(seqs, merges, kernel_ms=ms)
    assert same(first, second) and len(ms) == 2 and all(t > 0.0 for t in ms)
