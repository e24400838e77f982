"""smx_nj on the GPU against its numpy twin (tests/tree_utils.py nj_reference), by == on the raw records: the doubles are
compared as bits.  Sizes at every edge of the kernels' shapes -- a wave of 64 lanes and four rows per workgroup in the
row-minimum kernel, 256 threads in the init kernel, 1024 threads in the join kernel -- and the matrices on which the
order of operations, the tie rule, the integer row sums and the workspace's reuse can go wrong."""
import functools

import numpy as np
import pytest

import tree_utils as U
from specimux_amd import calls

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(kind: str, n: int):
    """(the matrix's triangle, the twin's records), computed once per test run."""
    D = {"random": lambda: U.random_matrix_np(n, n), "equal": lambda: U.constant_matrix(n, 7),
         "zero": lambda: U.constant_matrix(n, 0), "ladder": lambda: U.ladder_matrix(n),
         "largest": lambda: U.constant_matrix(n, 2**31 - 1)}[kind]()
    tri, want = U.tri_of(D), U.nj_reference(D)
    for a in (tri,) + want:
        a.setflags(write=False)
    return tri, want


def check(kind, n):
    tri, want = case(kind, n)
    got = calls.nj(tri, n)
    assert U.same_records(got, want), (kind, n)
    return got


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_random_matrices(n):
    check("random", n)


@pytest.mark.parametrize("kind", ["equal", "zero"])
@pytest.mark.parametrize("n", [4, 6, 65, 257])
def test_every_q_ties(kind, n):
    merges, last, _ = check(kind, n)
    assert [(int(m["a"]), int(m["b"])) for m in merges] == [(0, 1)] + [(n + t - 1, n - t) for t in range(1, n - 3)]
    assert last.tolist() == [2 * n - 4, 3, 2]


def test_the_ladder_that_rounds():
    check("ladder", 80)


def test_the_largest_entries_keep_the_row_sums_exact():
    merges, _, _ = check("largest", 64)
    assert float(merges[0]["ra"]) == 63.0 * (2**31 - 1)


def test_an_additive_tree_of_2049_tips():
    """Above the twin's reach: checked by the bipartitions and the exact integer branch lengths of the generating tree."""
    n = 2049
    D, splits = U.additive_matrix(77, n)
    got = U.splits_of_result(n, *calls.nj(U.tri_of(D), n))
    assert got == splits


def test_no_stale_workspace():
    """A large call, then a small one, then the small one alone: the workspace the large call grew and filled changes
    nothing."""
    check("random", 1025)
    after = check("random", 65)
    alone = check("random", 65)
    assert U.same_records(after, alone)
    check("zero", 65)                               # and zeros over what the random call left
    check("random", 9)


def test_the_same_call_twice():
    tri, _ = case("ladder", 80)
    ms = []
    first, second = calls.nj(tri, 80, ms), calls.nj(tri, 80, ms)
    assert U.same_records(first, second)
    assert len(ms) == 2 and all(t > 0.0 for t in ms)
