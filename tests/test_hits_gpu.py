"""The identify kernel on the GPU (smx_hits.hip): smx_best_hits_distances against the suite's oracle under the pair rule
over patterns of every state class and the generic one, on both sides, windows of 1 / 127 / 128 / 129 / 257 texts, limits
at d - 1, d, d + 1 and none, coverage at the threshold and one byte short, identical targets, jobs sharing targets;
smx_best_hits == the sorted reference for K = 1, 3 and 16; 300 offers to one row and 300 rows with one offer each; two calls
give the same keys; a small call after a large one; refusals launch nothing."""
import random

import numpy as np
import pytest

from oracle.edlib_semantics import HW, align_c
from specimux_amd import _lib, calls, identify

pytestmark = pytest.mark.gpu

LENGTHS = (1, 63, 64, 65, 128, 129, 200, 300, 500, 700, 1024, 1025, 1100)
COV = 300


def rand_seq(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def mutate(rng, s, rate, alpha="ACGT"):
    out = []
    for c in s:
        r = rng.random()
        if r < rate / 3:
            out.append(rng.choice(alpha))
        elif r < 2 * rate / 3:
            out.append(c + rng.choice(alpha))
        elif r >= rate:
            out.append(c)
    return "".join(out) or s


def build_case(seed=5):
    """Job 0: a query per state class against a family of targets per query -- flanked (the query is the pattern), trimmed
    (the target is), of equal length, mutated, a stranger -- and a twin of the first target at the end.  Then one job per
    window size on each side, short sequences; a job that shares the targets of the 257 window; jobs without queries and
    without targets.  edge[i] in (-1, 0, 1): sequence i's limit becomes (its smallest distance as a pattern) + that."""
    rng = random.Random(seed)
    alpha = "ACGTN"
    seqs, ks, edge, jobs = [], [], [], []

    def add(s, k, e=None):
        seqs.append(s)
        ks.append(k)
        edge.append(e)
        return len(seqs) - 1

    def limit(s):
        return -1 if rng.randrange(9) == 0 else len(s) // 8

    roots = [rand_seq(rng, m, alpha) for m in LENGTHS]
    for r in roots:
        add(r, limit(r), rng.choice((None, None, -1, 0, 1)))
    nq = len(seqs)
    for r in roots:
        m = len(r)
        a, b = rng.randrange(m // 4 + 1), m - rng.randrange(m // 4 + 1)
        fam = [rand_seq(rng, rng.randrange(61), alpha) + r + rand_seq(rng, 1 + rng.randrange(60), alpha),
               rand_seq(rng, 1 + rng.randrange(60), alpha) + mutate(rng, r, 0.04, alpha) + rand_seq(rng, rng.randrange(61), alpha),
               r[a:max(b, a + 1)], mutate(rng, r[a:max(b, a + 1)], 0.04, alpha), r, mutate(rng, r, 0.08, alpha),
               rand_seq(rng, m, alpha), rand_seq(rng, max(1, (m * 1000) // COV), alpha), rand_seq(rng, (m * 1000) // COV + 1, alpha)]
        for t in fam:
            add(t, limit(t), rng.choice((None, None, None, -1, 0, 1)))
    add(seqs[nq], ks[nq])
    jobs.append((0, nq, nq, len(seqs) - nq))
    shared = None
    for n in (1, 127, 128, 129, 257):              # side Q: one query of 40, n longer targets
        q = rand_seq(rng, 40)
        q0 = add(q, 5, rng.choice((-1, 0, 1)))
        t0 = len(seqs)
        for i in range(n):
            core = rand_seq(rng, 40) if i % 3 == 2 else mutate(rng, q, 0.01 * rng.randrange(20))
            add(rand_seq(rng, 1 + rng.randrange(15)) + core + rand_seq(rng, 6 + rng.randrange(10)), 4)
        jobs.append((q0, 1, t0, n))
        shared = (t0, n)
    for n in (1, 127, 128, 129, 257):              # side T: one target of 30, n longer queries
        t = rand_seq(rng, 30)
        t0 = add(t, 4, rng.choice((-1, 0, 1)))
        q0 = len(seqs)
        for i in range(n):
            core = rand_seq(rng, 30) if i % 3 == 2 else mutate(rng, t, 0.01 * rng.randrange(20))
            add(rand_seq(rng, 1 + rng.randrange(15)) + core + rand_seq(rng, 6 + rng.randrange(10)), 4)
        jobs.append((q0, n, t0, 1))
    extra = add(rand_seq(rng, 40), -1)
    jobs.append((extra, 1) + shared)               # jobs sharing targets
    jobs.append((0, 0) + shared)                   # no queries
    lone = add(rand_seq(rng, 12), 3)
    jobs.append((lone, 1, 0, 0))                   # no targets: its row stays empty
    return seqs, ks, edge, jobs


def reference(seqs, ks, edge, jobs, cov):
    """The unlimited oracle distance of every eligible pair (once), the limits of the edge sequences from them, and then
    per job the nq x nt matrix expected of the device."""
    full = []
    dmin = {}
    for q0, nq, t0, nt in jobs:
        d = np.full((nq, nt), -2, dtype=np.int64)  # -2: excluded by coverage
        for q in range(q0, q0 + nq):
            for t in range(t0, t0 + nt):
                q_is_pattern, ok = identify.pair_rule(len(seqs[q]), len(seqs[t]), cov)
                if ok:
                    p, x = (q, t) if q_is_pattern else (t, q)
                    d[q - q0, t - t0] = align_c(seqs[p], seqs[x], HW, -1, iupac=False)["editDistance"]
                    dmin[p] = min(dmin.get(p, 1 << 30), int(d[q - q0, t - t0]))
        full.append(d)
    ks = list(ks)
    for i, e in enumerate(edge):
        if e is not None and i in dmin:
            ks[i] = max(0, dmin[i] + e)
    want, near = [], {-1: 0, 0: 0, 1: 0, "none": 0, "excluded": 0, "q": 0, "t": 0}
    for (q0, nq, t0, nt), d in zip(jobs, full):
        w = np.full((nq, nt), -1, dtype=np.int32)
        for q in range(nq):
            for t in range(nt):
                if d[q, t] == -2:
                    near["excluded"] += 1
                    continue
                q_is_pattern = len(seqs[q0 + q]) <= len(seqs[t0 + t])
                near["q" if q_is_pattern else "t"] += 1
                k = ks[q0 + q] if q_is_pattern else ks[t0 + t]
                w[q, t] = d[q, t] if k < 0 or d[q, t] <= k else -1
                near["none" if k < 0 else k - int(d[q, t])] = near.get("none" if k < 0 else k - int(d[q, t]), 0) + 1
        want.append(w)
    return ks, want, near


def keys_from(seqs, jobs, want, K):
    rows = []
    for (q0, nq, t0, nt), w in zip(jobs, want):
        for q in range(nq):
            offers = sorted(identify.pack_key(int(w[q, t]), min(len(seqs[q0 + q]), len(seqs[t0 + t])), t)
                            for t in range(nt) if w[q, t] >= 0)
            rows.append((offers + [identify.NONE] * K)[:K])
    return np.array(rows, dtype=np.uint64).reshape(-1)


@pytest.fixture(scope="module")
def case():
    seqs, ks, edge, jobs = build_case()
    ks, want, near = reference(seqs, ks, edge, jobs, COV)
    assert min(near[-1], near[0], near[1]) >= 20 and near["none"] >= 100 and near["excluded"] >= 100, near
    assert near["q"] >= 800 and near["t"] >= 500, near
    return [s.encode("latin-1") for s in seqs], ks, jobs, want


def test_distances_match_the_oracle(case):
    seqs, ks, jobs, want = case
    got = identify.best_hits_distances(seqs, ks, jobs, 5, COV)
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and not (g == -7).any(), j
        bad = np.argwhere(g != w)
        assert bad.size == 0, (j, jobs[j], bad[:5].tolist(), [(int(g[q, t]), int(w[q, t])) for q, t in bad[:5]])
    assert sum(int((w >= 0).sum()) for w in want) >= 600 and sum(int((w < 0).sum()) for w in want) >= 500


def test_distances_walk_over_many_short_records():
    """The chunk walk (smx_mine_lds.h) where it can go wrong, all in state class 1: 4201 jobs of one short query each over
    windows of 1, 129 and 257 longer targets of a shared set, more than 4096 records, so that the owner search takes its
    third round; records of one, two and three chunks in turn, so that most workgroups of 8 chunks start inside a
    record; a chunk total that is no multiple of 8.  The sequences are drawn from two small pools, so the oracle aligns
    every distinct pair once; every distance of the call is compared."""
    rng = random.Random(6)
    qpool = [rand_seq(rng, rng.randrange(12, 21)) for _ in range(48)]
    kpool = [rng.choice((-1, 1, 3, 6)) for _ in qpool]
    tpool = [rand_seq(rng, rng.randrange(21, 41)) if i % 2 else
             (rand_seq(rng, rng.randrange(9)) + mutate(rng, qpool[i], 0.1) + rand_seq(rng, 20))[:rng.randrange(23, 41)]
             for i in range(48)]
    assert all(identify.pair_rule(len(q), len(t), COV) == (True, True) for q in qpool for t in tpool)
    table = np.empty((48, 48), dtype=np.int32)
    for a, (q, k) in enumerate(zip(qpool, kpool)):
        for b, t in enumerate(tpool):
            d = align_c(q, t, HW, -1, iupac=False)["editDistance"]
            table[a, b] = d if k < 0 or d <= k else -1
    n_t, n_rec = 600, 4201
    tid = np.array([rng.randrange(48) for _ in range(n_t)])
    qid = [rng.randrange(48) for _ in range(n_rec)]
    jobs = [(n_t + i, 1, rng.randrange(300), (1, 129, 257)[i % 3]) for i in range(n_rec)]
    starts = np.concatenate([[0], np.cumsum([(j[3] + 127) // 128 for j in jobs])])      # the records' chunk prefix
    first = np.arange(0, starts[-1], 8)                                                # every workgroup's first chunk
    assert starts[-1] % 8 != 0 and np.isin(first, starts, invert=True).mean() > 0.5
    seqs = [tpool[x].encode("latin-1") for x in tid] + [qpool[x].encode("latin-1") for x in qid]
    ks = [4] * n_t + [kpool[x] for x in qid]
    got = identify.best_hits_distances(seqs, ks, jobs, 5, COV)
    assert len(got) == n_rec
    n_in = n_out = 0
    for i, (g, (_, _, t0, nt)) in enumerate(zip(got, jobs)):
        w = table[qid[i], tid[t0:t0 + nt]].reshape(1, nt)
        bad = np.argwhere(g != w)
        assert g.shape == w.shape and bad.size == 0, (i, jobs[i], bad[:5].tolist(), [(int(g[q, t]), int(w[q, t])) for q, t in bad[:5]])
        n_in, n_out = n_in + int((w >= 0).sum()), n_out + int((w < 0).sum())
    assert n_in > 50000 and n_out > 50000


@pytest.mark.parametrize("K", [1, 3, 16])
def test_keys_equal_the_sorted_reference(case, K):
    seqs, ks, jobs, want = case
    keys = identify.best_hits(seqs, ks, jobs, K, COV)
    ref = keys_from(seqs, jobs, want, K)
    assert keys.shape == ref.shape and (keys == ref).all(), np.argwhere(keys != ref)[:5].tolist()
    rows = keys.reshape(-1, K)
    filled = (rows != np.uint64(identify.NONE)).sum(axis=1)
    assert (filled == 0).sum() >= 3 and (filled == K).sum() >= 2             # empty rows, full rows
    if K > 1:
        assert ((filled > 0) & (filled < K)).sum() >= 3                       # and rows in between
    again = identify.best_hits(seqs, ks, jobs, K, COV)
    assert (again == keys).all()                   # two calls give identical keys


@pytest.fixture(scope="module")
def contention():
    """Side Q: one query of 50 and 300 near-identical longer targets (three chunks offer to one row).  Side T: 300 queries
    that hold one short target (one row each, the same target index)."""
    rng = random.Random(9)
    q = rand_seq(rng, 50)
    seqs, ks = [q], [8]
    for i in range(300):
        seqs.append("AC" + mutate(rng, q, 0.02 * (i % 4)) + "GT" + "A" * (i % 3))
        ks.append(3)
    t = rand_seq(rng, 30)
    seqs.append(t)
    ks.append(2)
    for i in range(300):
        seqs.append(rand_seq(rng, 3 + i % 5) + mutate(rng, t, 0.03 * (i % 3)) + rand_seq(rng, 4))
        ks.append(9)
    jobs = [(0, 1, 1, 300), (302, 300, 301, 1)]
    _, want, _ = reference(seqs, ks, [None] * len(seqs), jobs, 0)
    assert (want[0] >= 0).sum() >= 250 and (want[1] >= 0).sum() >= 150
    return [s.encode("latin-1") for s in seqs], ks, jobs, want


@pytest.mark.parametrize("K", [3, 16])
def test_many_offers_to_one_row(contention, K):
    seqs, ks, jobs, want = contention
    ref = keys_from([s.decode("latin-1") for s in seqs], jobs, want, K)
    for _ in range(2):
        keys = identify.best_hits(seqs, ks, jobs, K, 0)
        assert (keys == ref).all(), np.argwhere(keys != ref)[:5].tolist()
    assert (keys[:K] != np.uint64(identify.NONE)).all()


def test_a_small_call_after_a_large_one(case, contention):
    seqs, ks, jobs, want = case
    identify.best_hits(seqs, ks, jobs, 16, COV)    # grows the workspace
    small = [b"ACGTACGTAC", b"TTACGTACGTACTT", b"ACGAACGTAC", b"GGGGGGGGGGGG"]
    keys = identify.best_hits(small, [1, 1, 1, 1], [(0, 1, 1, 3)], 4, 0)
    assert [int(x) for x in keys] == [identify.pack_key(0, 10, 0), identify.pack_key(1, 10, 1), identify.NONE, identify.NONE]
    d = identify.best_hits_distances(small, [1, 1, 1, 1], [(0, 1, 1, 3)], 4, 0)
    assert d[0].tolist() == [[0, 1, -1]]


def test_refusals_launch_nothing():
    lib = _lib.load()
    seqs = [b"ACGTACGT", b"ACGAACGT", b"", b"ACGT", b"ACGTT"]
    off = calls.offsets(seqs)
    ks = np.array([2] * len(seqs), dtype=np.int32)

    def call(jobs, K=5, cov=500):
        jarr = np.array(jobs, dtype=_lib.HITS_JOB_DTYPE)
        a = np.full(256, 0x5A, dtype=np.uint64)
        ms = _lib.C.c_float(-1.0)                  # its own kernel_ms, and so a direct call: a refusal must leave it alone
        rc = lib.smx_best_hits(b"".join(seqs), _lib.ptr(off), len(seqs), _lib.ptr(ks), _lib.ptr(jarr), len(jobs), K, cov,
                               _lib.ptr(a), _lib.C.byref(ms))
        return rc, lib.smx_last_error().decode(), a, ms.value
    for jobs, kw, word in (([(1, 2, 3, 2)], {}, "empty"), ([(0, 2, 2, 2)], {}, "empty"), ([(0, 6, 3, 1)], {}, "out of bounds"),
                           ([(0, 2, 3, 1), (1, 1, 4, 1)], {}, "overlap"), ([(0, 2, 3, 2)], {"K": 17}, "K = 17"),
                           ([(0, 2, 3, 2)], {"cov": 1001}, "min_cov_permille")):
        rc, msg, a, ms = call(jobs, **kw)
        assert rc == _lib.ERR_ARG and word in msg, (jobs, rc, msg)
        assert (a == 0x5A).all() and ms == -1.0    # neither the keys nor the kernel time were touched
    big = bytes(300) + bytes(range(256)) * 60      # 256 distinct bytes x 245 words: the Peq table does not fit the LDS
    boff = np.array([0, len(big), 2 * len(big) + 1], dtype=np.uint64)
    jarr = np.array([(0, 1, 1, 1)], dtype=_lib.HITS_JOB_DTYPE)
    a = np.full(16, 0x5A, dtype=np.uint64)
    rc = lib.smx_best_hits(big + big + b"A", _lib.ptr(boff), 2, _lib.ptr(np.array([5, 5], dtype=np.int32)), _lib.ptr(jarr), 1, 5, 0,
                           _lib.ptr(a), None)
    assert rc == _lib.ERR_UNSUPPORTED and "LDS" in lib.smx_last_error().decode() and (a == 0x5A).all()
    # shared targets: both jobs over sequences 3 and 4, each the pattern of its pairs
    rc, msg, a, ms = call([(0, 1, 3, 2), (1, 1, 3, 2)], K=2, cov=0)
    assert rc == _lib.OK, msg
    want = identify.best_hits_oracle(seqs, [2] * len(seqs), [(0, 1, 3, 2), (1, 1, 3, 2)], 2, 0)
    assert (a[:4] == want).all() and int(want[0]) == identify.pack_key(0, 4, 0) and int(want[1]) == identify.pack_key(1, 5, 1)
    assert ms >= 0.0
