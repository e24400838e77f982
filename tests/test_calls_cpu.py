"""specimux_amd.calls against a recording stand-in for libsmx: what every one-shot call is handed (argument count and
order, dtypes, bytes, the sentinel its outputs hold on entry), what comes back (shapes and contents), the device time and
the status.  The expected arguments are written out by hand from include/smx.h; nothing here needs libsmx.so or a GPU."""
import ctypes as C

import numpy as np
import pytest

from specimux_amd import _lib, calls

MS = 1.25                                    # the device time the fake reports
KEY, WORD = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
JOB4 = np.dtype([("q0", "<u4"), ("nq", "<u4"), ("t0", "<u4"), ("nt", "<u4")])       # smx_nearest_job, smx_hits_job, smx_reach_job
MINE_JOB = np.dtype([("q0", "<u4"), ("nq", "<u4"), ("t0", "<u4"), ("nt", "<u4"), ("min_identity", "<f8")])
PAIRS_JOB = np.dtype([("r0", "<u4"), ("n", "<u4")])
CONS_JOB = np.dtype([("draft", "<u4"), ("r0", "<u4"), ("n", "<u4")])
SITE = np.dtype([("pos", "<u4"), ("kind", "u1"), ("major", "u1"), ("minor", "u1"), ("pad", "u1"), ("n_major", "<u4"),
                 ("n_minor", "<u4")])


class Out:
    """An output argument as the test expects it: `count` entries of `dtype` that hold `sentinel` on entry (None: not
    prefilled).  The fake writes `fill`, by default a pattern that depends on the position and on the argument."""

    def __init__(self, dtype, count, sentinel, fill=None):
        self.dtype, self.count, self.sentinel, self.fill = np.dtype(dtype), count, sentinel, fill
        self.written = None

    @property
    def nbytes(self):
        return self.count * self.dtype.itemsize


class FakeLib:
    """Every smx_* attribute records its arguments -- the bytes behind each pointer, the value of each scalar -- fills the
    outputs, reports MS as the device time and returns `status`.  `layout` (one entry per argument before kernel_ms: an
    array or an Out for a pointer, anything else for a value) only tells it how many bytes each pointer stands for."""

    def __init__(self, status=0):
        self.status, self.layout, self.log = status, [], []

    def smx_last_error(self):
        return b"refused by the fake"

    def __getattr__(self, name):
        if not name.startswith("smx_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        seen = []
        for pos, arg in enumerate(args[:-1]):
            spec = self.layout[pos] if pos < len(self.layout) else None
            if not isinstance(arg, C.c_void_p):
                seen.append(arg)
                continue
            assert arg.value, f"{name}: argument {pos} is a null pointer"
            assert isinstance(spec, (np.ndarray, Out)), f"{name}: argument {pos} is a pointer"
            seen.append(C.string_at(arg.value, spec.nbytes))
            if isinstance(spec, Out):
                fill = spec.fill if spec.fill is not None else (np.arange(spec.count) * 3 + pos + 1)
                spec.written = np.array(fill).astype(spec.dtype).reshape(spec.count)
                C.memmove(arg.value, spec.written.ctypes.data, spec.nbytes)
        args[-1]._obj.value = MS
        self.log.append((name, seen))
        return self.status


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    return lib


def call(fake, name, layout, fn, *args):
    """fn(*args, kernel_ms) through the fake: checks the one recorded call against `layout` and the device time, then the
    same call with kernel_ms=None.  Returns what fn returned."""
    fake.layout, ms = layout, []
    got = fn(*args, ms)
    assert ms == [MS]
    (seen_name, seen), = fake.log
    assert seen_name == name
    assert len(seen) == len(layout), "argument count (kernel_ms apart)"
    for pos, (arg, spec) in enumerate(zip(seen, layout)):
        where = f"{name}: argument {pos}"
        if isinstance(spec, np.ndarray):
            assert arg == spec.tobytes(), where
        elif isinstance(spec, Out):
            if spec.sentinel is not None:
                assert arg == np.full(spec.count, spec.sentinel, dtype=spec.dtype).tobytes(), where
        else:
            assert type(arg) is type(spec) and arg == spec, where
    fn(*args, None)                              # kernel_ms=None: nothing to append to, the call is made all the same
    assert len(fake.log) == 2 and ms == [MS]
    return got


def same(got, want, shape=None):
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == (want.shape if shape is None else shape)
    assert np.array_equal(got.reshape(-1), want.reshape(-1))


def u64(*v):
    return np.array(v, dtype="<u8")


def u32(*v):
    return np.array(v, dtype="<u4")


def i32(*v):
    return np.array(v, dtype="<i4")


# five sequences, an empty one between two others, and the five limits of the issue: below zero, zero, the largest int32,
# and two that do not fit
S = [b"ACGT", b"", b"GG", b"TTTAA", b"C"]
S_BLOB, S_OFF = b"ACGTGGTTTAAC", u64(0, 4, 4, 6, 11, 12)
KS = [-5, 0, 2**31 - 1, 2**31, 2**40]
K_ARR = i32(-1, 0, 2147483647, 2147483647, 2147483647)
T = [b"AC", b"", b"GGG"]
T_BLOB, T_OFF = b"ACGGG", u64(0, 2, 2, 5)
JOBS4 = [(0, 2, 2, 3), (0, 0, 1, 0), (3, 1, 0, 2)]          # nq x nt = 2 x 3, 0 x 0, 1 x 2
JOBS4_ARR = np.array(JOBS4, dtype=JOB4)
CONS_JOBS = [(0, 0, 2), (3, 2, 0), (1, 2, 3)]               # drafts of 4, 5 and 0 bases; 2, 0 and 3 members
CONS_JOBS_ARR = np.array(CONS_JOBS, dtype=CONS_JOB)
CONS_HEAD = [S_BLOB, S_OFF, 5, K_ARR, CONS_JOBS_ARR, 3]
EMPTY_HEAD = [b"", u64(0), 0, i32()]


# ------------------------------------------------------------------------------------------------ the helpers
def test_offsets():
    same(calls.offsets([]), u64(0))
    same(calls.offsets(S), S_OFF)
    same(calls.offsets([b"AC", b"", b"G"], np.uint32), u32(0, 2, 2, 3))


def test_limits():
    same(calls.limits(KS), K_ARR)
    same(calls.limits([]), i32())


def test_job_array():
    for jobs in ([], ()):
        arr = calls.job_array(jobs, JOB4)
        assert arr.dtype == JOB4 and arr.shape == (0,) and arr.ctypes.data
    arr = calls.job_array(JOBS4, JOB4)
    assert arr.dtype == JOB4 and arr.tobytes() == u32(0, 2, 2, 3, 0, 0, 1, 0, 3, 1, 0, 2).tobytes()
    assert calls.job_array([(1, 2, 3, 4, 0.5)], MINE_JOB).tobytes() == u32(1, 2, 3, 4).tobytes() + np.float64(0.5).tobytes()


def test_split():
    flat = np.arange(10, dtype=np.int32)
    a, b, c, d = calls.split(flat, [(2, 2), (0, 3), 1, (1, 2, 2)])
    same(a, i32(0, 1, 2, 3), (2, 2))
    same(b, i32(), (0, 3))
    same(c, i32(4), (1,))
    same(d, i32(5, 6, 7, 8), (1, 2, 2))
    assert a.base is flat                     # views, not copies
    assert calls.split(flat, []) == []


def test_invoke(fake):
    ms = []
    assert calls.invoke("smx_anything", 7, b"x", None, kernel_ms=ms) == 0
    assert fake.log == [("smx_anything", [7, b"x", None])] and ms == [MS]
    assert calls.invoke("smx_anything", kernel_ms=None) == 0
    fake.status = -2
    with pytest.raises(_lib.SmxError) as e:
        calls.invoke("smx_anything", 1)
    assert e.value.code == -2 and "refused by the fake" in str(e.value)
    assert calls.invoke("smx_anything", 1, kernel_ms=ms, check=False) == -2
    assert ms == [MS, MS]


# ------------------------------------------------------------------------------------------------ specimine
MINE_JOBS = [(0, 2, 0, 1, 0.85), (2, 3, 1, 0, 0.5), (0, 5, 1, 2, 0.9)]      # nq x nt = 2 x 1, 3 x 0, 5 x 2
MINE_HEAD = [S_BLOB, S_OFF, 5, K_ARR, T_BLOB, T_OFF, 3, np.array(MINE_JOBS, dtype=MINE_JOB), 3]
MINE_EMPTY = [b"", u64(0), 0, i32(), b"", u64(0), 0, np.zeros(0, dtype=MINE_JOB), 0]


def test_mine_best_identity(fake):
    best = Out("<f8", 3, 0.0)
    got = call(fake, "smx_mine_best_identity", MINE_HEAD + [best], calls.mine_best_identity, S, KS, T, MINE_JOBS)
    same(got, best.written)


def test_mine_best_identity_empty(fake):
    best = Out("<f8", 1, 0.0)
    got = call(fake, "smx_mine_best_identity", MINE_EMPTY + [best], calls.mine_best_identity, [], [], [], [])
    assert got.shape == (1,)                  # the floor itself: specimine never makes the call without jobs


def test_mine_distances(fake):
    dist = Out("<i4", 12, -7)
    a, b, c = call(fake, "smx_mine_distances", MINE_HEAD + [dist], calls.mine_distances, S, KS, T, MINE_JOBS)
    same(a, dist.written[0:2], (2, 1))
    same(b, i32(), (3, 0))
    same(c, dist.written[2:12], (5, 2))


def test_mine_distances_empty(fake):
    assert call(fake, "smx_mine_distances", MINE_EMPTY + [Out("<i4", 1, -7)], calls.mine_distances, [], [], [], []) == []


# ------------------------------------------------------------------------------------------------ clusters
PAIRS_JOBS = [(0, 2), (2, 0), (2, 3)]
PAIRS_HEAD = [S_BLOB, S_OFF, 5, K_ARR, np.array(PAIRS_JOBS, dtype=PAIRS_JOB), 3]
PAIRS_EMPTY = EMPTY_HEAD + [np.zeros(0, dtype=PAIRS_JOB), 0]


def test_pairs_neighbours(fake):
    adj = Out("<u4", 5, 0)                    # 2 x 1, 0 x 0 and 3 x 1 words
    a, b, c = call(fake, "smx_pairs_neighbours", PAIRS_HEAD + [adj], calls.pairs_neighbours, S, KS, PAIRS_JOBS)
    same(a, adj.written[0:2], (2, 1))
    same(b, u32(), (0, 0))
    same(c, adj.written[2:5], (3, 1))


def test_pairs_neighbours_two_words(fake):
    reads = [b"A"] * 33                       # 33 reads: two words per row
    head = [b"A" * 33, np.arange(34, dtype="<u8"), 33, np.zeros(33, dtype="<i4"), np.array([(0, 33)], dtype=PAIRS_JOB), 1]
    adj = Out("<u4", 66, 0)
    a, = call(fake, "smx_pairs_neighbours", head + [adj], calls.pairs_neighbours, reads, [0] * 33, [(0, 33)])
    same(a, adj.written, (33, 2))


def test_pairs_distances(fake):
    dist = Out("<i4", 4, -7)                  # triangles of 1, 0 and 3 pairs
    a, b, c = call(fake, "smx_pairs_distances", PAIRS_HEAD + [dist], calls.pairs_distances, S, KS, PAIRS_JOBS)
    same(a, dist.written[0:1])
    same(b, i32())
    same(c, dist.written[1:4])


def test_pairs_empty(fake):
    assert call(fake, "smx_pairs_neighbours", PAIRS_EMPTY + [Out("<u4", 1, 0)], calls.pairs_neighbours, [], [], []) == []
    fake.log.clear()
    assert call(fake, "smx_pairs_distances", PAIRS_EMPTY + [Out("<i4", 1, -7)], calls.pairs_distances, [], [], []) == []


# ------------------------------------------------------------------------------------------------ consensus and its kin
CONS_EMPTY = EMPTY_HEAD + [np.zeros(0, dtype=CONS_JOB), 0]


def test_cons_votes(fake):
    votes, aligned = Out("<u4", 312, 0), Out("<u4", 3, 0)          # (5 + 6 + 1) rows of 26 words
    tables, n = call(fake, "smx_cons_votes", CONS_HEAD + [votes, aligned], calls.cons_votes, S, KS, CONS_JOBS)
    same(tables[0], votes.written[0:130], (5, 26))
    same(tables[1], votes.written[130:286], (6, 26))
    same(tables[2], votes.written[286:312], (1, 26))
    assert len(tables) == 3 and n == [int(x) for x in aligned.written] and all(type(x) is int for x in n)


def test_cons_votes_empty(fake):
    layout = CONS_EMPTY + [Out("<u4", 1, 0), Out("<u4", 1, 0)]
    assert call(fake, "smx_cons_votes", layout, calls.cons_votes, [], [], []) == ([], [])


def test_cons_pileup(fake):
    rows, dist = Out("<u4", 13, WORD), Out("<i4", 5, -7)            # 2 x 5, 0 x 6 and 3 x 1 words; 2 + 0 + 3 members
    r, d = call(fake, "smx_cons_pileup", CONS_HEAD + [rows, dist], calls.cons_pileup, S, KS, CONS_JOBS)
    same(r[0], rows.written[0:10], (2, 5))
    same(r[1], u32(), (0, 6))
    same(r[2], rows.written[10:13], (3, 1))
    same(d[0], dist.written[0:2])
    same(d[1], i32())
    same(d[2], dist.written[2:5])


def test_cons_pileup_empty(fake):
    layout = CONS_EMPTY + [Out("<u4", 1, WORD), Out("<i4", 1, -7)]
    assert call(fake, "smx_cons_pileup", layout, calls.cons_pileup, [], [], []) == ([], [])


def test_cons_phase(fake):
    site_fill = np.array([(p, p & 1, 1, 2, 0, 10 + p, 5 + p) for p in range(6)], dtype=SITE)
    votes, aligned, sites = Out("<u4", 312, 0), Out("<u4", 3, 0), Out(SITE, 6, 0, site_fill)    # 3 jobs x 2 slots
    n_sites, n_qual = Out("<u4", 3, 0, [1, 0, 2]), Out("<u4", 3, 0)
    planes, link = Out("<u8", 8, 0), Out("<u4", 48, 0)        # (1 + 0 + 1) words x 2 x 2 slots; 3 x 2 x 2 x 4
    layout = CONS_HEAD + [150, 5, 2, votes, aligned, sites, n_sites, n_qual, planes, link]
    got = call(fake, "smx_cons_phase", layout, calls.cons_phase, S, KS, CONS_JOBS, 150, 5, 2)
    assert len(got) == 3 and all(len(job) == 6 for job in got)
    for j, (lo, hi, rows) in enumerate(((0, 130, 5), (130, 286, 6), (286, 312, 1))):
        same(got[j][0], votes.written[lo:hi], (rows, 26))
        assert got[j][1] == int(aligned.written[j]) and got[j][3] == int(n_qual.written[j])
        same(got[j][5], link.written[16 * j:16 * j + 16], (2, 2, 4))
    assert [[int(s["pos"]) for s in got[j][2]] for j in range(3)] == [[0], [], [4, 5]]
    assert [int(s["n_minor"]) for s in got[2][2]] == [9, 10] and got[2][2].dtype == SITE
    same(got[0][4], planes.written[0:4], (2, 2, 1))
    same(got[1][4], u64(), (2, 2, 0))
    same(got[2][4], planes.written[4:8], (2, 2, 1))


def test_cons_phase_empty(fake):
    layout = CONS_EMPTY + [150, 5, 64] + [Out("<u4", 1, 0), Out("<u4", 1, 0), Out(SITE, 1, 0, np.zeros(1, SITE)), Out("<u4", 1, 0),
                                          Out("<u4", 1, 0), Out("<u8", 1, 0), Out("<u4", 1, 0)]
    assert call(fake, "smx_cons_phase", layout, calls.cons_phase, [], [], [], 150, 5, 64) == []


def test_cons_resample(fake):
    masks = np.arange(10, dtype=np.uint64).reshape(2, 5) + np.uint64(2**63)         # 2 levels x (2 + 0 + 3) members
    votes, aligned = Out("<u4", 312, 0), Out("<u4", 3, 0)
    agree, sub = Out("<u8", 24, 0), Out("<u4", 384, 0)        # 2 levels x (5 + 6 + 1) columns; 3 jobs x 2 levels x 64
    layout = CONS_HEAD + [u64(*range(2**63, 2**63 + 10)), 2, votes, aligned, agree, sub]
    got = call(fake, "smx_cons_resample", layout, calls.cons_resample, S, KS, CONS_JOBS, masks)
    assert len(got) == 3 and all(len(job) == 4 for job in got)
    for j, (lo, hi, rows) in enumerate(((0, 130, 5), (130, 286, 6), (286, 312, 1))):
        same(got[j][0], votes.written[lo:hi], (rows, 26))
        assert got[j][1] == int(aligned.written[j])
        same(got[j][3], sub.written[128 * j:128 * j + 128], (2, 64))
    same(got[0][2], agree.written[0:10], (2, 5))
    same(got[1][2], agree.written[10:22], (2, 6))
    same(got[2][2], agree.written[22:24], (2, 1))


def test_cons_resample_no_levels(fake):
    votes, aligned = Out("<u4", 312, 0), Out("<u4", 3, 0)
    layout = CONS_HEAD + [None, 0, votes, aligned, Out("<u8", 1, 0), Out("<u4", 1, 0)]       # a null masks pointer
    got = call(fake, "smx_cons_resample", layout, calls.cons_resample, S, KS, CONS_JOBS, np.zeros((0, 5), dtype=np.uint64))
    assert [job[2].shape for job in got] == [(0, 5), (0, 6), (0, 1)] and [job[3].shape for job in got] == [(0, 64)] * 3
    same(got[2][0], votes.written[286:312], (1, 26))


def test_cons_resample_empty(fake):
    layout = CONS_EMPTY + [None, 2, Out("<u4", 1, 0), Out("<u4", 1, 0), Out("<u8", 1, 0), Out("<u4", 1, 0)]
    assert call(fake, "smx_cons_resample", layout, calls.cons_resample, [], [], [], np.zeros((2, 0), dtype=np.uint64)) == []


@pytest.mark.parametrize("masks", [np.zeros((2, 4), np.uint64), np.zeros((2, 6), np.uint64), np.zeros(5, np.uint64)])
def test_cons_resample_refuses_masks_of_another_shape(fake, masks):
    with pytest.raises(ValueError):
        calls.cons_resample(S, KS, CONS_JOBS, masks)
    assert fake.log == []                     # before the library is called


# ------------------------------------------------------------------------------------------------ crosstalk
GROUPS = [0, 1, 1, 2, 7]
NEAREST_HEAD = [S_BLOB, S_OFF, 5, K_ARR, u32(0, 1, 1, 2, 7), JOBS4_ARR, 3]
NEAREST_EMPTY = EMPTY_HEAD + [u32(), np.zeros(0, dtype=JOB4), 0]


def test_nearest(fake):
    own, other = Out("<u8", 5, KEY), Out("<u8", 5, KEY)        # one key per read: nt = 3 + 0 + 2
    a, b = call(fake, "smx_nearest", NEAREST_HEAD + [own, other], calls.nearest, S, KS, GROUPS, JOBS4)
    same(a, own.written)
    same(b, other.written)


def test_nearest_empty(fake):
    a, b = call(fake, "smx_nearest", NEAREST_EMPTY + [Out("<u8", 1, KEY), Out("<u8", 1, KEY)], calls.nearest, [], [], [], [])
    same(a, u64())
    same(b, u64())


def test_nearest_distances(fake):
    dist = Out("<i4", 8, -7)
    a, b, c = call(fake, "smx_nearest_distances", NEAREST_HEAD + [dist], calls.nearest_distances, S, KS, GROUPS, JOBS4)
    same(a, dist.written[0:6], (2, 3))
    same(b, i32(), (0, 0))
    same(c, dist.written[6:8], (1, 2))


def test_nearest_distances_empty(fake):
    assert call(fake, "smx_nearest_distances", NEAREST_EMPTY + [Out("<i4", 1, -7)], calls.nearest_distances, [], [], [], []) == []


# ------------------------------------------------------------------------------------------------ identify
HITS_HEAD = [S_BLOB, S_OFF, 5, K_ARR, JOBS4_ARR, 3]
HITS_EMPTY = EMPTY_HEAD + [np.zeros(0, dtype=JOB4), 0]


def test_best_hits(fake):
    keys = Out("<u8", 9, KEY)                  # K = 3 keys per query: nq = 2 + 0 + 1
    got = call(fake, "smx_best_hits", HITS_HEAD + [3, 500, keys], calls.best_hits, S, KS, JOBS4, 3, 500)
    same(got, keys.written)


def test_best_hits_without_slots(fake):
    got = call(fake, "smx_best_hits", HITS_HEAD + [0, 500, Out("<u8", 1, KEY)], calls.best_hits, S, KS, JOBS4, 0, 500)
    same(got, u64())


def test_best_hits_empty(fake):
    same(call(fake, "smx_best_hits", HITS_EMPTY + [5, 0, Out("<u8", 1, KEY)], calls.best_hits, [], [], [], 5, 0), u64())


def test_best_hits_distances(fake):
    dist = Out("<i4", 8, -7)
    a, b, c = call(fake, "smx_best_hits_distances", HITS_HEAD + [3, 500, dist], calls.best_hits_distances, S, KS, JOBS4, 3, 500)
    same(a, dist.written[0:6], (2, 3))
    same(b, i32(), (0, 0))
    same(c, dist.written[6:8], (1, 2))


def test_best_hits_distances_empty(fake):
    layout = HITS_EMPTY + [5, 0, Out("<i4", 1, -7)]
    assert call(fake, "smx_best_hits_distances", layout, calls.best_hits_distances, [], [], [], 5, 0) == []


# ------------------------------------------------------------------------------------------------ bimera
WEIGHTS, NEEDS = [1, 2**32 - 1, 2**32, 2**40, 0], [0, 3, 2**33, 1, 2]              # above the cap: 2^32 - 1
REACH_HEAD = [S_BLOB, S_OFF, 5, u32(1, 4294967295, 4294967295, 4294967295, 0), u32(0, 3, 4294967295, 1, 2), JOBS4_ARR, 3]
REACH_EMPTY = [b"", u64(0), 0, u32(), u32(), np.zeros(0, dtype=JOB4), 0]


def test_prefix_reach_no_edits(fake):
    keys = Out("<u8", 12, KEY)                 # E = 0: 3 queries x 2 sides x 1 x 2 slots
    got = call(fake, "smx_prefix_reach", REACH_HEAD + [0, keys], calls.prefix_reach, S, WEIGHTS, NEEDS, JOBS4, 0)
    same(got, keys.written)


def test_prefix_reach(fake):
    keys = Out("<u8", 36, KEY)                 # E = 2: 3 queries x 2 sides x 3 x 2 slots
    got = call(fake, "smx_prefix_reach", REACH_HEAD + [2, keys], calls.prefix_reach, S, WEIGHTS, NEEDS, JOBS4, 2)
    same(got, keys.written)


def test_prefix_reach_empty(fake):
    same(call(fake, "smx_prefix_reach", REACH_EMPTY + [0, Out("<u8", 1, KEY)], calls.prefix_reach, [], [], [], [], 0), u64())


def test_prefix_reach_matrix(fake):
    vals = Out("<u4", 48, WORD)                # E = 2: (6 + 0 + 2) pairs x 2 sides x 3
    a, b, c = call(fake, "smx_prefix_reach_matrix", REACH_HEAD + [2, vals], calls.prefix_reach_matrix, S, WEIGHTS, NEEDS, JOBS4, 2)
    same(a, vals.written[0:36], (2, 3, 2, 3))
    same(b, u32(), (0, 0, 2, 3))
    same(c, vals.written[36:48], (1, 2, 2, 3))


def test_prefix_reach_matrix_no_edits(fake):
    vals = Out("<u4", 16, WORD)
    a, b, c = call(fake, "smx_prefix_reach_matrix", REACH_HEAD + [0, vals], calls.prefix_reach_matrix, S, WEIGHTS, NEEDS, JOBS4, 0)
    same(a, vals.written[0:12], (2, 3, 2, 1))
    same(c, vals.written[12:16], (1, 2, 2, 1))


def test_prefix_reach_matrix_empty(fake):
    layout = REACH_EMPTY + [0, Out("<u4", 1, WORD)]
    assert call(fake, "smx_prefix_reach_matrix", layout, calls.prefix_reach_matrix, [], [], [], [], 0) == []


# ------------------------------------------------------------------------------------------------ chimera
PATTERNS = ["ACG", "", "TT"]                   # an empty pattern between two others
PATTERN_ARGS = [b"ACGTT", u32(0, 3, 3, 5), 3, i32(1, 0, 2)]
BASES, READ_OFF = np.frombuffer(b"ACGTAC", dtype=np.uint8), u64(0, 4, 6)


class Batch:
    handle = 0xBEEF

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def scan_outputs(n, q, h):
    return [Out("u1", n * q, None), Out("i1", n * q * h, None), Out("<i4", n * q * h, None)]


def check_scan(got, outs, n, q, h):
    same(got[0], outs[0].written, (n, q))
    same(got[1], outs[1].written, (n, q, h))
    same(got[2], outs[2].written, (n, q, h))


def test_inner_scan(fake):
    outs = scan_outputs(2, 3, 2)
    layout = PATTERN_ARGS + [BASES, READ_OFF, 2, 10, 2, 4096] + outs
    check_scan(call(fake, "smx_inner_scan", layout, calls.inner_scan, BASES, [0, 4, 6], PATTERNS, [1, 0, 2], 10, 2, 4096), outs, 2, 3, 2)


def test_inner_scan_no_reads_one_pattern(fake):
    outs = scan_outputs(0, 1, 4)
    layout = [b"ACG", u32(0, 3), 1, i32(1), np.zeros(0, dtype=np.uint8), u64(0), 0, 3, 4, 0] + outs
    got = call(fake, "smx_inner_scan", layout, calls.inner_scan, np.zeros(0, dtype=np.uint8), [0], ["ACG"], [1], 3, 4, 0)
    check_scan(got, outs, 0, 1, 4)


def test_inner_scan_batch(fake):
    outs = scan_outputs(3, 3, 1)
    layout = [0xBEEF] + PATTERN_ARGS + [0, 1, 0] + outs
    check_scan(call(fake, "smx_inner_scan_batch", layout, calls.inner_scan_batch, Batch(3), PATTERNS, [1, 0, 2], 0, 1, 0), outs, 3, 3, 1)


# ------------------------------------------------------------------------------------------------ the status
M0 = np.zeros((0, 0), dtype=np.uint64)
ENTRY_POINTS = {
    "smx_mine_best_identity": lambda ms: calls.mine_best_identity([], [], [], [], ms),
    "smx_mine_distances": lambda ms: calls.mine_distances([], [], [], [], ms),
    "smx_pairs_neighbours": lambda ms: calls.pairs_neighbours([], [], [], ms),
    "smx_pairs_distances": lambda ms: calls.pairs_distances([], [], [], ms),
    "smx_cons_votes": lambda ms: calls.cons_votes([], [], [], ms),
    "smx_cons_pileup": lambda ms: calls.cons_pileup([], [], [], ms),
    "smx_cons_phase": lambda ms: calls.cons_phase([], [], [], 150, 5, 8, ms),
    "smx_cons_resample": lambda ms: calls.cons_resample([], [], [], M0, ms),
    "smx_nearest": lambda ms: calls.nearest([], [], [], [], ms),
    "smx_nearest_distances": lambda ms: calls.nearest_distances([], [], [], [], ms),
    "smx_best_hits": lambda ms: calls.best_hits([], [], [], 5, 0, ms),
    "smx_best_hits_distances": lambda ms: calls.best_hits_distances([], [], [], 5, 0, ms),
    "smx_prefix_reach": lambda ms: calls.prefix_reach([], [], [], [], 0, ms),
    "smx_prefix_reach_matrix": lambda ms: calls.prefix_reach_matrix([], [], [], [], 0, ms),
    "smx_inner_scan": lambda ms: calls.inner_scan(np.zeros(1, np.uint8), [0, 1], ["A"], [0], 0, 1, 0, ms),
    "smx_inner_scan_batch": lambda ms: calls.inner_scan_batch(Batch(1), ["A"], [0], 0, 1, 0, ms),
}


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_status(fake, monkeypatch, name):
    """A nonzero status raises SmxError out of the typed function; invoke(..., check=False) hands the same status back."""
    monkeypatch.setattr(FakeLib, "_call", lambda self, fn, args: (self.log.append(fn), setattr(args[-1]._obj, "value", MS),
                                                                  self.status)[2])
    fake.status = _lib.ERR_UNSUPPORTED
    ms = []
    with pytest.raises(_lib.SmxError) as e:
        ENTRY_POINTS[name](ms)
    assert e.value.code == _lib.ERR_UNSUPPORTED and fake.log == [name] and ms == []
    assert calls.invoke(name, kernel_ms=ms, check=False) == _lib.ERR_UNSUPPORTED and ms == [MS]
    fake.status = 0
    ENTRY_POINTS[name](ms)
    assert ms == [MS, MS]
