"""The device aligner (smx_align, smx_align_batch: specimux_amd/csrc/smx_align.hip) where its byte-wide score column, its
start rule and its workspace could go wrong: targets far longer than 256 letters, k >= m, k = 250, location caps below the
location count, launches whose last wave is full, partial or one lane, calls of very different sizes one after another, and
align_seq's slices.  Everything is compared exactly with oracle.edlib_semantics.align (align_seq: specimux_oracle.align_seq).
tests/test_align_cpu.py runs the same kernel bodies on the CPU over far more cases; the refusals are tested there."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WRAP_M = (1, 2, 6, 7, 20, 58, 63, 64)


@pytest.fixture(scope="module")
def lib():
    from specimux_amd import _lib
    lib = _lib.load()
    n = C.c_int(0)
    _lib.check(lib.smx_device_init(0, C.byref(n)))
    assert n.value >= 1
    return lib


@functools.lru_cache(maxsize=None)
def oracle_any_k(q, t, mode):
    from oracle import edlib_semantics as E
    r = E.align(q, t, E.SHW if mode else E.HW, -1)
    return r["editDistance"], [tuple(x) for x in r["locations"]]


def oracle(q, t, k, mode):
    """(distance, locations) of edlib_semantics.align(q, t, mode, k): k only decides whether the best distance counts."""
    d, locs = oracle_any_k(q, t, mode)
    return (d, locs) if d <= k else (-1, [])


def single(lib, q, t, k, mode, cap=None):
    """smx_align -> (dist, nloc, the pairs written); cap None: room for every column, cap 0: NULL buffers."""
    from specimux_amd import _lib
    cap = len(t) if cap is None else cap
    starts, ends = ((C.c_int * cap)(), (C.c_int * cap)()) if cap else (None, None)
    dist, nloc = C.c_int(), C.c_int()
    _lib.check(lib.smx_align(q.encode(), len(q), t.encode("latin-1"), len(t), k, mode, C.byref(dist), starts, ends, cap, C.byref(nloc)))
    return dist.value, nloc.value, [(starts[i], ends[i]) for i in range(min(nloc.value, cap))]


def batch(lib, reqs, cap):
    """smx_align_batch over (q, t, k, mode) -> per request (dist, nloc, the pairs written); cap 0: NULL buffers."""
    from specimux_amd import _lib, calls
    qtab = {}
    qidx = np.array([qtab.setdefault(r[0], len(qtab)) for r in reqs], dtype=np.uint32)
    qoff, toff = calls.offsets(list(qtab), np.uint32), calls.offsets([r[1] for r in reqs])
    k, mode = np.array([r[2] for r in reqs], dtype=np.int32), np.array([r[3] for r in reqs], dtype=np.uint8)
    n = len(reqs)
    dist, nloc = np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int32)
    starts, ends = (np.full((n, cap), -7, dtype=np.int32), np.full((n, cap), -7, dtype=np.int32)) if cap else (None, None)
    _lib.check(lib.smx_align_batch("".join(qtab).encode(), _lib.ptr(qoff), len(qtab), "".join(r[1] for r in reqs).encode("latin-1"),
                                   _lib.ptr(toff), _lib.ptr(qidx), _lib.ptr(k), _lib.ptr(mode), n, _lib.ptr(dist), _lib.ptr(nloc),
                                   _lib.ptr(starts), _lib.ptr(ends), cap))
    return [(int(dist[i]), int(nloc[i]), [(int(starts[i, j]), int(ends[i, j])) for j in range(min(int(nloc[i]), cap))]) for i in range(n)]


def expected(req, cap):
    d, locs = oracle(*req)
    return d, len(locs), locs[:cap]


def wrap_query(m):
    rng = random.Random(1000 + m)
    q = [rng.choice("AG") for _ in range(m)]
    if m >= 6:
        q[m // 2] = "R"          # `C` and `x` match none of its letters
    return "".join(q)


def wrap_targets(q, n):
    """The families of tests/cpu/align_sim.cpp: the query then filler, half the query then filler, no matching letter, two
    letters of which the query holds one.  The first is a wrap witness by construction where n >= m + 256."""
    m, fill = len(q), "Cx"[n % 2]
    rng = random.Random(m * 7919 + n)
    return [(q + fill * n)[:n], (q[:m // 2] + fill * n)[:n], "".join("x" if i % 3 == 0 else "C" for i in range(n)),
            "".join(rng.choice("AC") for _ in range(n))]


# ------------------------------------------------------------------ the byte-wide column through smx_align
def test_witness_of_the_byte_wide_column_has_one_location(lib):
    """q = A, t = A then 300 C, k = 0, SHW: column 256 costs 256, which a byte holds as 0 = best."""
    assert single(lib, "A", "A" + "C" * 300, 0, 1) == (0, 1, [(0, 0)]) == expected(("A", "A" + "C" * 300, 0, 1), 301)


@pytest.mark.parametrize("mode", [0, 1])
def test_single_call_on_targets_past_256_columns(lib, mode):
    from oracle import edlib_semantics as E
    reqs, constructed = [], []
    for m in WRAP_M:
        q = wrap_query(m)
        for n in sorted({255, 256, 257, m + 255, m + 256, 600, 1000}):
            for f, t in enumerate(wrap_targets(q, n)):
                for k in sorted({0, m - 1, m, 250, 1000}):
                    reqs.append((q, t, k, mode))
                if f == 0 and n >= m + 256:
                    constructed.append((q, t))
    # by the oracle alone: the query then at least 256 letters of filler costs 0 as a prefix alignment, and its column
    # m + 256 costs 256 -- equal to best in a byte.  Three target lengths per query length reach that far.
    assert len(constructed) == 8 * 3
    for q, t in constructed:
        assert E.align(q, t, E.SHW, -1)["editDistance"] == 0
        assert E.align(q, t[:len(q) + 256], E.NW, -1)["editDistance"] == 256
    for r in reqs:
        assert single(lib, *r) == expected(r, len(r[1])), (r[0], len(r[1]), r[1][:70], r[2], r[3])
    assert len(reqs) > 8 * 5 * 4 * 4


def test_single_call_hw_on_a_5000_letter_target(lib):
    """Copies of the query at column 0, inside and ending at the last column, two more with a substitution: *nloc is the
    true count whatever cap is, and the first min(nloc, cap) pairs are the oracle's first."""
    rng = random.Random(5000)
    q = "".join(rng.choice("ACGT") for _ in range(24))
    t = [rng.choice("ACGT") for _ in range(5000)]
    for pos in (0, 777, 2500, 4000, 5000 - 24):
        t[pos:pos + 24] = q
    for pos in (1500, 3333):
        t[pos:pos + 24] = q[:11] + ("A" if q[11] != "A" else "C") + q[12:]
    t = "".join(t)
    for k in (0, 1, 24):
        d, locs = oracle(q, t, k, 0)
        assert d == 0 and len(locs) >= 5 and locs[0] == (0, 23) and locs[-1] == (4976, 4999)
        for cap in (0, 1, len(locs)):
            assert single(lib, q, t, k, 0, cap) == (d, len(locs), locs[:cap]), (k, cap)
    # one letter that every base matches: 5000 optimal ends
    d, locs = oracle("N", t, 0, 0)
    assert len(locs) == 5000
    for cap in (1, 4999, 5000):
        assert single(lib, "N", t, 0, 0, cap) == (0, 5000, locs[:cap])


# ------------------------------------------------------------------ k >= m
def test_k_at_and_above_the_query_length(lib):
    """best = m is then within k: a target without a matching letter has every column optimal in HW mode, and the start
    rule's backward scan runs its full m + best columns.  Both entries, both modes."""
    rng = random.Random(77)
    reqs = []
    for m in (1, 5, 32, 33, 64):
        q = "".join(rng.choice("ACGTACGTACGTNRYKMSWBDHV") for _ in range(m))
        ordinary = "".join(rng.choice("ACGTACGTNax") for _ in range(100))
        pos = rng.randrange(0, 100 - m)
        copy = "".join(c if rng.random() > 0.1 else rng.choice("ACGT") for c in q)
        targets = ["x?xa-" * 8, ordinary[:pos] + copy + ordinary[pos + m:], ordinary]
        targets += [copy[:n] for n in sorted({1, max(m // 2, 1), max(m - 1, 1)})]       # shorter than the query, down to 1
        for t in targets:
            for k in (m, m + 1, 64, 250):
                for mode in (0, 1):
                    reqs.append((q, t, k, mode))
    barren = [r for r in reqs if r[1].startswith("x?xa-") and r[3] == 0]
    assert all(oracle(*r) == (len(r[0]), [(max(e - len(r[0]) + 1, 0), e) for e in range(40)]) for r in barren)
    for r in reqs:
        assert single(lib, *r) == expected(r, len(r[1])), r
    cap = max(len(oracle(*r)[1]) for r in reqs)
    assert cap >= 40
    assert batch(lib, reqs, cap) == [expected(r, cap) for r in reqs]


# ------------------------------------------------------------------ smx_align_batch at its largest k
@pytest.fixture(scope="module")
def wrap_requests():
    """The wrap families at k = 250, both modes: 8 query lengths x 6 target lengths x 4 targets x 2 modes."""
    reqs = []
    for m in WRAP_M:
        q = wrap_query(m)
        for n in sorted({m + 249, m + 250, m + 251, 257, m + 256, 1000}):
            for t in wrap_targets(q, n):
                reqs += [(q, t, 250, 0), (q, t, 250, 1)]
    random.Random(3).shuffle(reqs)
    return reqs


@pytest.mark.parametrize("n", [1, 64, 65, 129])
def test_batch_at_k_250_by_launch_size(lib, wrap_requests, n):
    """The last wave of 64 lanes is full (64), holds one lane (1, 65, 129) -- and every lane's target runs past 256 columns."""
    reqs = wrap_requests[n:2 * n]
    cap = max(len(oracle(*r)[1]) for r in reqs)
    assert batch(lib, reqs, cap) == [expected(r, cap) for r in reqs]


def test_batch_at_k_250_lengths_and_queries(lib, wrap_requests):
    rng = random.Random(250)
    # one wave: target lengths from 1 to 1000, modes mixed, queries of the wrap families
    wave = []
    for i in range(64):
        q = wrap_query(WRAP_M[i % 8])
        n = 1 + (999 * i) // 63
        wave.append((q, wrap_targets(q, n)[i % 4], 250, (i // 3) % 2))
    assert {len(r[1]) for r in wave} >= {1, 1000} and {r[3] for r in wave} == {0, 1}
    # every lane on one query; every lane on a query of its own
    q = wrap_query(58)
    same = [(q, "".join(rng.choice("ACGx") for _ in range(rng.randint(1, 400))), 250, i % 2) for i in range(100)]
    queries = set()
    while len(queries) < 70:
        queries.add("".join(rng.choice("ACGTN") for _ in range(1 + len(queries) % 64)))
    own = [(qi, "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 330))), 250, i % 2) for i, qi in enumerate(sorted(queries))]
    for reqs in (wave, same, own, wrap_requests[300:400]):
        cap = max(len(oracle(*r)[1]) for r in reqs)
        assert batch(lib, reqs, cap) == [expected(r, cap) for r in reqs]


# ------------------------------------------------------------------ the location cap
@pytest.fixture(scope="module")
def cap_requests():
    """A one-letter `N` query against plain bases has every column optimal: 40 locations, more than align_batch's first guess
    of 16.  Beside it: one, a few and no locations."""
    rng = random.Random(16)
    t40 = "".join(rng.choice("ACGT") for _ in range(40))
    reqs = [("N", t40, 0, 0), ("N", t40[:17], 0, 0), ("N", t40, 0, 1), ("ACGT", "ACGTTTACGTACGA", 0, 0), ("ACGT", "ACGTTTACGTACGA", 1, 0),
            ("ACGT", "TTTTTTTT", 1, 0), ("AC", "ACACACACACACACACACACACACACACACACACACAC", 0, 0), ("A", "C", 1, 0)]
    reqs += [("ACGTN", "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 60))), rng.choice((0, 1, 2, 5)), i % 2) for i in range(60)]
    assert len(oracle(*reqs[0])[1]) == 40 == max(len(oracle(*r)[1]) for r in reqs)
    return reqs


@pytest.mark.parametrize("cap", [0, 1, 39, 40])
def test_batch_location_cap(lib, cap_requests, cap):
    """nloc is the true count; the first min(nloc, cap) pairs are the oracle's first; cap 0 takes NULL buffers."""
    assert batch(lib, cap_requests, cap) == [expected(r, cap) for r in cap_requests]


def test_align_batch_regrows_past_its_first_cap(lib, cap_requests):
    from specimux_amd.alignment import align_batch
    got = align_batch([(q, t, k, ("HW", "SHW")[mode]) for q, t, k, mode in cap_requests])
    assert [(d, [tuple(x) for x in locs]) for d, locs in got] == [oracle(*r) for r in cap_requests]


# ------------------------------------------------------------------ the grow-only workspace
def test_results_do_not_depend_on_the_calls_before(lib):
    rng = random.Random(100)

    def request(i, longest):
        q = "".join(rng.choice("ACGTACGTN") for _ in range(rng.choice((1, 7, 20, 33, 64))))
        return q, "".join(rng.choice("ACGTax") for _ in range(rng.randint(1, longest))), rng.choice((0, 3, len(q), 250)), i % 2
    small = [request(i, 120) for i in range(100)]
    large = [request(i, 300) for i in range(5000)]
    first = batch(lib, small, 8)
    assert first == [expected(r, 8) for r in small]
    assert len(batch(lib, large, 3)) == 5000
    assert batch(lib, small, 8) == first


# ------------------------------------------------------------------ align_seq's slices
@pytest.mark.parametrize("mode", ["HW", "SHW"])
def test_align_seq_slices_against_the_oracle(lib, mode):
    """Negative starts, -1, ends beyond the sequence and empty targets, directly and through an AlignCache.  On an empty target
    the reference keeps edlib's one location (None, -1) and clamps the distance; where the query is within k of the empty
    string its shift adds a number to None: the oracle raises the reference's TypeError, and so must align_seq."""
    from oracle import specimux_oracle as O
    from specimux_amd.alignment import AlignCache, align_seq
    rng = random.Random(9)
    query = "ACGTNA"
    seq = "".join(rng.choice("ACGT") for _ in range(12)) + "ACGTCA" + "".join(rng.choice("ACGTn") for _ in range(13))
    L = len(seq)
    grid = [(k, s, e) for k in (1, 6, 9) for s in (-1, 0, 5, -10, -(L + 3), L, L + 2) for e in (-1, 3, L, L + 5)]
    cache, keys = AlignCache(), []
    for k, s, e in grid:
        t = seq[(0 if s == -1 else s):(L if e == -1 else min(e, L))]
        if t:
            keys.append((query, t[:len(query) + k] if mode == "SHW" else t, k, mode))
    cache.fill(keys)
    assert set(keys) == set(cache.table) and len(cache.table) >= 3 * 3      # three k, at least the slices from 0, 5 and -10
    n_empty = n_raise = 0
    for k, s, e in grid:
        try:
            exp = O.align_seq(query, seq, k, s, e, mode)
        except TypeError:
            exp = None
        for use_cache in (False, True):
            try:
                if use_cache:
                    with cache:
                        got = align_seq(query, seq, k, s, e, mode)
                else:
                    got = align_seq(query, seq, k, s, e, mode)
                got = (got.distance(), [tuple(x) for x in got.locations()])
            except TypeError:
                got = None
            assert got == (None if exp is None else (exp.dist, [tuple(x) for x in exp.locs])), (k, s, e, use_cache)
        n_empty += exp is not None and exp.locs == [(None, -1)]
        n_raise += exp is None
    assert n_empty >= 10 and n_raise >= 10
