"""flank_assign_kernel (specimux_amd/csrc/smx_flank.hip) against a plain twin of its own (tests/flank_utils.py: the key
layout of include/smx.h, the suite's edlib oracle for the distance, the best / first / ntied rule in plain Python), at the
edges of its launch: a caller's candidate list that the host has to regroup, keys in any order, key counts around the
256-lane workgroup, candidate lists around the 256-candidate LDS chunk with ties across the chunk boundary, candidates
and flanks of every length, k = 0 and k >= m, IUPAC candidates, the matched bit.  Every comparison is == on all three
arrays, and every test asserts on the twin's own output that its fixture reaches the edge it is after."""
import ctypes as C

import numpy as np
import pytest

from flank_utils import assign_reference, key_parts, make_key, shw_distance

pytestmark = pytest.mark.gpu
CHUNK, LANES = 256, 256          # FLANK_ACHUNK, FLANK_THREADS (smx_flank_core.h)


@pytest.fixture(scope="module")
def lib():
    from specimux_amd import _lib
    lib = _lib.load()
    n = C.c_int(0)
    _lib.check(lib.smx_device_init(0, C.byref(n)))
    assert n.value >= 1
    return lib


def seq(rng, n, letters="ACGT"):
    return "".join(letters[c] for c in rng.integers(0, len(letters), n))


def mutate(rng, s, edits):
    """`edits` random substitutions, insertions and deletions."""
    s = list(s)
    for _ in range(edits):
        kind, at = int(rng.integers(3)), int(rng.integers(len(s) + 1))
        if kind == 0 and s:
            at %= len(s)
            s[at] = "ACGT"[("ACGT".index(s[at]) + 1 + int(rng.integers(3))) % 4]
        elif kind == 1:
            s.insert(at, "ACGT"[int(rng.integers(4))])
        elif s:
            del s[at % len(s)]
    return "".join(s)


def instance(rng, cand):
    """A plain string the IUPAC candidate equals letter by letter."""
    sets = {"N": "ACGT", "R": "AG", "Y": "CT"}
    return "".join(ch if ch in "ACGT" else sets[ch][int(rng.integers(len(sets[ch])))] for ch in cand)


def planted(rng, cand, edits, tail=3):
    return (mutate(rng, instance(rng, cand), edits) + seq(rng, tail))[:26]


def check(keys, cands, k):
    """The kernel against the twin on all three arrays; returns the twin's (best, first, ntied) and its distance lists."""
    from specimux_amd import barcodes
    keys = np.array(keys, dtype=np.uint64)
    stats = {}
    want = assign_reference(keys, cands, k, stats)
    got = barcodes.assign(keys, cands, k)
    for g, w, name in zip(got, want, ("best", "first", "ntied")):
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (name, len(bad), [(int(i), key_parts(keys[i]), int(g[i]), int(w[i])) for i in bad[:5]])
    return want, stats.get("dists", {})


# ------------------------------------------------------------------------------------------------ caller's order
@pytest.fixture(scope="module")
def interleaved():
    """Candidates of primers 5, 0 and 63 interleaved in the caller's list (sizes that cross a chunk for primer 0), and keys
    of those primers and of primer 7, which has none.  Shared by the order tests; nothing changes it."""
    rng = np.random.default_rng(101)
    cands = []
    for i in range(600):
        p = (5, 0, 63)[i % 3] if i < 120 else (0 if i % 2 else 63)       # primer 5: 40, primers 0 and 63: 280 each
        cands.append((p, seq(rng, 13)))
    keys = []
    for p in (0, 5, 63):
        mine = [s for q, s in cands if q == p]
        for i in range(230):
            src = mine[int(rng.integers(len(mine)))]
            flank = planted(rng, src, int(rng.integers(4))) if i % 5 else seq(rng, 16)
            keys.append(make_key(flank, i & 1, p))
    keys += [make_key(seq(rng, 16), 0, 7) for _ in range(30)]
    keys += keys[:40]                                                    # duplicate keys
    return cands, sorted(keys)


def test_candidates_in_the_callers_order(lib, interleaved):
    cands, keys = interleaved
    (best, first, ntied), _d = check(keys, cands, 3)
    order = sorted(range(len(cands)), key=lambda c: cands[c][0])         # stable: the grouping the host makes
    grouped = {c: s for s, c in enumerate(order)}
    found = [int(f) for f in first if f >= 0]
    assert len(found) >= 400
    assert sum(grouped[f] != f for f in found) >= 300                    # a kernel that returned the grouped index fails
    assert all(cands[f][0] == key_parts(key)[2] for f, key in zip(first, keys) if f >= 0)
    per_primer = {p: [c for c in range(len(cands)) if cands[c][0] == p] for p in (0, 63)}
    assert any(f in per_primer[0][CHUNK:] for f in found) and any(f in per_primer[63][CHUNK:] for f in found)   # second chunks
    none = [i for i, key in enumerate(keys) if key_parts(key)[2] == 7]
    assert len(none) == 30
    assert all((best[i], first[i], ntied[i]) == (-1, -1, 0) for i in none)


def test_keys_in_any_order(lib, interleaved):
    cands, keys = interleaved
    keys = np.array(keys, dtype=np.uint64)
    assert len(set(keys.tolist())) < len(keys)                           # duplicates
    base, _d = check(keys, cands, 3)
    rng = np.random.default_rng(7)
    n = len(keys)
    primer = np.array([key_parts(key)[2] for key in keys])
    # every block of 256 keys starts with a key of primer 0 and ends with one of primer 63
    lo, hi = list(np.flatnonzero(primer == 0)), list(np.flatnonzero(primer == 63))
    blocks = (n + LANES - 1) // LANES
    ends = set(lo[:blocks] + hi[:blocks])
    rest = [i for i in rng.permutation(n) if i not in ends]
    spread = []
    for b in range(blocks):
        size = min(LANES, n - b * LANES)
        spread += [lo[b]] + [rest.pop() for _ in range(size - 2)] + [hi[b]]
    assert not rest and sorted(spread) == list(range(n))
    for b in range(blocks):
        block = primer[spread[b * LANES:(b + 1) * LANES]]
        assert block.min() == 0 and block.max() == 63
    for name, perm in (("reversed", np.arange(n)[::-1]), ("shuffled", rng.permutation(n)), ("spread", np.array(spread))):
        want, _d = check(keys[perm], cands, 3)
        for w, b in zip(want, base):
            assert np.array_equal(w, b[perm]), name                      # the results permute with the keys


@pytest.mark.parametrize("n_keys", [1, 255, 256, 257, 513])
def test_key_counts_around_the_workgroup(lib, interleaved, n_keys):
    cands, keys = interleaved
    rng = np.random.default_rng(n_keys)
    take = [keys[i] for i in rng.permutation(len(keys))[:n_keys]]
    (best, _f, _n), _d = check(take, cands, 3)
    if n_keys > 1:
        assert (best >= 0).any() and (best < 0).any()
    if n_keys == 1:                                                      # and the single key is one with an answer
        one = next(key for key in keys if key_parts(key)[2] == 63)
        (best, first, _n), _d = check([one], cands, 26)
        assert best[0] >= 0 and cands[first[0]][0] == 63


# ------------------------------------------------------------------------------------------------ chunks
@pytest.mark.parametrize("n_cands", [1, 255, 256, 257, 600])
def test_candidates_per_primer_around_the_chunk(lib, n_cands):
    """Primer 3 has n_cands candidates; five candidates of primer 9 stand in front of them in the caller's list, so that a
    caller's index is the grouped index + 5.  k = 1: random 13-mers are further apart than that."""
    rng = np.random.default_rng(1000 + n_cands)
    k, front = 1, [(9, seq(rng, 13)) for _ in range(5)]
    mine = [seq(rng, 13) for _ in range(n_cands)]
    keys, expect = [], []
    x = seq(rng, 13)
    if n_cands > CHUNK:                                                  # equal distances on both sides of the chunk boundary
        mine[CHUNK - 1] = x[:3] + "ACGT"[("ACGT".index(x[3]) + 1) % 4] + x[4:]
        mine[CHUNK] = x[:8] + "ACGT"[("ACGT".index(x[8]) + 2) % 4] + x[9:]
        keys.append(make_key(x + seq(rng, 3), 0, 3))
        expect.append((1, 5 + CHUNK - 1, 2))
    if n_cands == 600:                                                   # one candidate three times, once per chunk
        mine[300] = mine[590] = mine[10]
        keys.append(make_key(mine[10] + seq(rng, 3), 1, 3))
        expect.append((0, 5 + 10, 3))
    for at in sorted({0, min(CHUNK - 1, n_cands - 1), min(CHUNK, n_cands - 1), n_cands - 1}):
        keys.append(make_key(mine[at] + seq(rng, 3), 0, 3))              # the only candidate within k sits at `at`
        expect.append((0, 5 + at, 1))
    keys += [make_key(planted(rng, mine[int(rng.integers(n_cands))], int(rng.integers(3))), 0, 3) for _ in range(40)]
    keys += [make_key(front[2][1] + "ACG", 0, 9)]
    expect.append((0, 2, 1))
    cands = front + [(3, s) for s in mine]
    (best, first, ntied), _d = check(keys, cands, k)
    got = list(zip(best.tolist(), first.tolist(), ntied.tolist()))
    assert got[:len(expect) - 1] == expect[:-1] and got[-1] == expect[-1], (got[:len(expect)], expect)
    if n_cands > CHUNK:
        assert any(f >= 5 + CHUNK for f in first)                        # an answer from the second chunk
    if n_cands == 600:
        assert any(f >= 5 + 2 * CHUNK for f in first)                    # and from the third


# ------------------------------------------------------------------------------------------------ lengths and k
@pytest.fixture(scope="module")
def lengths():
    """Candidates of 1, 8, 13, 16 and 26 letters mixed within primer 2 (a few with N, R, Y), and for each of them flanks
    of 0, 1, m - 3, m, m + 3 and 26 bases that are planted copies with 0..5 edits."""
    rng = np.random.default_rng(202)
    cands = []
    for rep in range(4):
        for m in (13, 1, 26, 8, 16):
            cands.append((2, seq(rng, m, "ACGTNRY" if rep == 3 else "ACGT")))
    keys, source = [], []
    for c, (_p, s) in enumerate(cands):
        m = len(s)
        for flen in sorted({0, 1, max(0, m - 3), m, min(26, m + 3), 26}):
            for edits in range(6):
                for _rep in range(2):
                    flank = (mutate(rng, instance(rng, s), edits) + seq(rng, 26))[:flen]
                    keys.append(make_key(flank, int(rng.integers(2)), 2))
                    source.append(c)
    return cands, keys, source


@pytest.mark.parametrize("k", [0, 1, 3, 26])
def test_lengths_and_thresholds(lib, lengths, k):
    cands, keys, source = lengths
    (best, first, ntied), dists = check(keys, cands, k)
    flens = {len(key_parts(key)[0]) for key in keys}
    assert {0, 1, 4, 5, 8, 10, 11, 13, 16, 19, 23, 26} <= flens
    assert {len(s) for _p, s in cands} == {1, 8, 13, 16, 26}
    d_src = np.array([dict(dists[i])[source[i]] for i in range(len(keys))])
    at_k, past_k = int((d_src == k).sum()), int((d_src == k + 1).sum())
    print(f"k={k}: {len(keys)} keys, planted copies at distance k: {at_k}, at k + 1: {past_k}, unassigned {(best < 0).sum()}")
    if k < 26:
        assert at_k >= 36 and past_k >= 36                               # planted copies exactly at and just past the threshold
        assert (best < 0).any() == (k == 0)                              # a 1-letter candidate is within 1 of anything
    else:
        # k >= m for every candidate: all of them qualify for every key, the empty flank included
        assert (best >= 0).all() and all(ntied[i] == sum(d == best[i] for _c, d in dists[i]) for i in range(len(keys)))
        assert max(d for i in dists for _c, d in dists[i]) == 26         # a 26-letter candidate against the empty flank
    empty = [i for i, key in enumerate(keys) if len(key_parts(key)[0]) == 0]
    assert len(empty) >= 100 and all(dict(dists[i])[source[i]] == len(cands[source[i]][1]) for i in empty)


def test_iupac_candidates_win_and_tie(lib):
    rng = np.random.default_rng(303)
    cands, keys, kind = [], [], []
    for i in range(60):
        x = seq(rng, 13)
        at = sorted(rng.permutation(13)[:3].tolist())
        deg = "".join({0: "N", 1: "R" if ch in "AG" else "Y", 2: "N"}[at.index(j)] if j in at else ch for j, ch in enumerate(x))
        if i % 3 == 0:
            cands += [(4, deg)]                                          # the IUPAC candidate alone: it wins
        elif i % 3 == 1:
            cands += [(4, x), (4, deg)]                                  # it ties with the plain one behind the plain one
        else:
            cands += [(4, deg), (4, x)]                                  # and in front of it
        for edits in (0, 0, 1, 2):
            keys.append(make_key(mutate(rng, x, edits) + seq(rng, 3), 1, 4))
            kind.append(i % 3)
    (best, first, ntied), dists = check(keys, cands, 3)
    iupac = [any(ch in "NRY" for ch in s) for _p, s in cands]
    wins = sum(1 for i in range(len(keys)) if first[i] >= 0 and iupac[first[i]])
    tie_partner = sum(1 for i in range(len(keys)) if ntied[i] >= 2 and not iupac[first[i]]
                      and any(iupac[c] and d == best[i] for c, d in dists[i]))
    print(f"IUPAC winners {wins}, IUPAC tie partners behind a plain winner {tie_partner}")
    assert wins >= 60 and tie_partner >= 30
    assert shw_distance("NRY", "AAC") == 0 and shw_distance("NRY", "ACA") == 1


def test_matched_bit_does_not_matter(lib, interleaved):
    cands, keys = interleaved
    flanks = sorted({key_parts(key)[0::2] for key in keys[::3]})
    clear = [make_key(f, 0, p) for f, p in flanks]
    both = clear + [make_key(f, 1, p) for f, p in flanks]
    (best, first, ntied), _d = check(both, cands, 3)
    n = len(clear)
    assert n >= 200 and (best >= 0).sum() >= 100
    assert np.array_equal(best[:n], best[n:]) and np.array_equal(first[:n], first[n:]) and np.array_equal(ntied[:n], ntied[n:])


def test_mixed_random_call(lib):
    """8 primers with 40-300 candidates each (13-mers, a few shorter, longer and IUPAC), about 2 000 keys in random order."""
    rng = np.random.default_rng(404)
    primers = [0, 1, 2, 7, 20, 31, 62, 63]
    sizes = [40, 300, 257, 120, 256, 64, 255, 180]
    cands = []
    for p, n in zip(primers, sizes):
        for _ in range(n):
            r = int(rng.integers(20))
            cands.append((p, seq(rng, 13) if r > 2 else seq(rng, (8, 16, 13)[r], "ACGTNRY" if r == 2 else "ACGT")))
    cands = [cands[i] for i in rng.permutation(len(cands))]              # primers interleaved at random
    keys = []
    for p in primers:
        mine = [s for q, s in cands if q == p]
        for i in range(250):
            src = mine[int(rng.integers(len(mine)))]
            keys.append(make_key(planted(rng, src, int(rng.integers(6)), tail=int(rng.integers(4))) if i % 6 else seq(rng, 16),
                                 int(rng.integers(2)), p))
    keys = [keys[i] for i in rng.permutation(len(keys))]
    (best, first, ntied), _d = check(keys, cands, 3)
    print(f"{len(keys)} keys, {len(cands)} candidates: {(best >= 0).sum()} assigned, {(ntied > 1).sum()} tied, "
          f"distances {np.bincount(best[best >= 0]).tolist()}")
    assert (best >= 0).sum() >= 1000 and (best < 0).sum() >= 100 and (ntied > 1).sum() >= 10
    assert set(best.tolist()) == {-1, 0, 1, 2, 3}
