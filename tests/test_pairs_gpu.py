"""The clusters kernel on the GPU (smx_pairs.hip through smx_pairs_distances / smx_pairs_neighbours): NW distances against
the O(m*n) oracle DP, the adjacency bit matrix against a host reduction of the distances, and the limits of the call."""
import random

import numpy as np
import pytest

from clusters_utils import mutate, rand_seq
from oracle.edlib_semantics import NW, align_c
from specimux_amd import _lib, calls

pytestmark = pytest.mark.gpu

ALL_BYTES = "".join(map(chr, range(256)))


def oracle_dist(a, b, k):
    """edlib NW by the suite's oracle.  The oracle reports max(m, n) for an empty side whatever k is; the ABI compares
    that distance with k like any other."""
    d = align_c(a, b, NW, k, iupac=False)["editDistance"]
    return -1 if (not a or not b) and 0 <= k < d else d


def pair_limit(ki, kj):
    return -1 if ki < 0 or kj < 0 else max(ki, kj)


def pairs_raw(reads, ks, jobs, neighbours=False, sentinel=None):
    """One smx_pairs_distances / smx_pairs_neighbours call on str reads; jobs are (r0, n).  The output is filled with a
    sentinel first.  -> (status, output array, kernel ms)."""
    rs = [r.encode("latin-1") for r in reads]
    roff, jarr = calls.offsets(rs), calls.job_array(jobs, _lib.PAIRS_JOB_DTYPE)
    if neighbours:
        n_out = sum(n * ((n + 31) // 32) for _, n in jobs)
        out = np.full(max(n_out, 1), 0xDEADBEEF if sentinel is None else sentinel, dtype=np.uint32)
        fn = "smx_pairs_neighbours"
    else:
        n_out = sum(n * (n - 1) // 2 for _, n in jobs)
        out = np.full(max(n_out, 1), -7 if sentinel is None else sentinel, dtype=np.int32)
        fn = "smx_pairs_distances"
    ms = []
    rc = calls.invoke(fn, b"".join(rs), _lib.ptr(roff), len(rs), _lib.ptr(np.array(ks, dtype=np.int32)), _lib.ptr(jarr), len(jobs),
                      _lib.ptr(out), kernel_ms=ms, check=False)
    return rc, out[:n_out], ms[0]


def job_pairs(jobs):
    """(i, j) global read indices in the order of smx_pairs_distances' output."""
    return [(r0 + i, r0 + j) for r0, n in jobs for i in range(n) for j in range(i + 1, n)]


def expected_dists(reads, ks, jobs):
    return np.array([oracle_dist(reads[i], reads[j], pair_limit(ks[i], ks[j])) for i, j in job_pairs(jobs)],
                    dtype=np.int64)


def assert_dists(reads, ks, jobs):
    rc, got, _ = pairs_raw(reads, ks, jobs)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    want = expected_dists(reads, ks, jobs)
    assert got.shape == want.shape
    pairs = job_pairs(jobs)
    bad = [(len(reads[pairs[x][0]]), len(reads[pairs[x][1]]), pair_limit(ks[pairs[x][0]], ks[pairs[x][1]]), int(got[x]),
            int(want[x])) for x in np.nonzero(got != want)[0]]
    assert not bad, f"{len(bad)} of {len(pairs)} pairs differ (m, n, k, kernel, oracle): {bad[:10]}"
    return want


def candidates(rng, q, k, alphabet):
    """A job around q, as test_specimine_gpu.py builds its candidates: a mutated copy, an identical read, one
    truncated beyond k, and end indels (the band drops blocks at the top / joins them at the bottom)."""
    m = len(q)
    kk = m if k < 0 else k
    core = mutate(rng, q, 0.08, alphabet) or q[:1]
    pick = rng.randrange(3)
    third = (q,                                                               # identical
             core[:max(1, m - kk - 1 - rng.randrange(3))],                     # shorter than m - k
             rand_seq(rng, rng.randrange(1, 40), alphabet) + core)[pick]       # an insertion at the very start
    tail = core[:max(1, len(core) - rng.randrange(1, 30))] if rng.random() < 0.5 else \
        core + rand_seq(rng, rng.randrange(1, 30), alphabet)                   # a deletion / an insertion at the very end
    return [q, core, third, tail][:rng.choice([3, 4])]


def test_distances_lengths_limits_alphabets():
    rng = random.Random(31)
    reads, ks, jobs = [], [], []
    for m in (1, 2, 63, 64, 65, 127, 128, 129, 200, 600, 1025, 1500, 4097):
        for k in (0, 3, int(0.15 * m), m + 5, -1):
            for alphabet in ("ACGT", "ACGTNRY", "ACGTacgtN") if m < 4097 else ("ACGT",):
                if m == 4097 and k != int(0.15 * m):
                    continue                                                  # the long one once
                job = candidates(rng, rand_seq(rng, m, alphabet), k, alphabet)
                jobs.append((len(reads), len(job)))
                reads += job
                ks += [k] * len(job)
    assert len(jobs) == 12 * 5 * 3 + 1 and sum(n * (n - 1) // 2 for _, n in jobs) > 700
    want = assert_dists(reads, ks, jobs)
    assert (want >= 0).sum() > 200 and (want == -1).sum() > 100 and (want == 0).sum() >= 20


def test_distances_mixed_limits_and_empty_reads():
    rng = random.Random(32)
    q = rand_seq(rng, 300)
    reads = [q, mutate(rng, q, 0.05), "", mutate(rng, q, 0.2), q[:280], "", "ACG", rand_seq(rng, 5000)]
    ks = [10, 40, 2, -1, 20, 400, 3, 4700]
    want = dict(zip(job_pairs([(0, len(reads))]), assert_dists(reads, ks, [(0, len(reads))])))
    assert want[(0, 2)] == -1 and want[(0, 5)] == 300                         # 300 against max(10, 2) and max(10, 400)
    assert want[(2, 5)] == 0 and want[(2, 6)] == 3 and want[(2, 3)] == len(reads[3])   # both empty; "" and ACG; no limit
    assert want[(0, 1)] == -1 or want[(0, 1)] <= 40


def test_distances_walk_over_many_short_rows():
    """The chunk walk (smx_mine_lds.h) where it can go wrong, all in state class 1: fourteen jobs of about 300 reads, more
    than 4096 rows, so that the owner search takes its third round; a job's rows own three, two and one chunk, so that
    most workgroups of 8 chunks start inside a row; a chunk total that is no multiple of 8.  The reads are drawn from a
    small pool, so the oracle aligns every distinct pair once; every distance of the call is compared."""
    rng = random.Random(33)
    pool = [rand_seq(rng, rng.randrange(12, 41)) for _ in range(24)]
    pool += [(mutate(rng, r, 0.1) or r)[:40].ljust(12, "A") for r in pool]
    kpool = [rng.choice((-1, 3, 6, 12)) for _ in pool]
    table = np.array([[oracle_dist(a, b, pair_limit(ka, kb)) for b, kb in zip(pool, kpool)] for a, ka in zip(pool, kpool)],
                     dtype=np.int64)
    sizes = [300 + (j * 7) % 11 - 5 for j in range(14)]
    ids = np.array([rng.randrange(len(pool)) for _ in range(sum(sizes))])
    jobs = [(sum(sizes[:j]), n) for j, n in enumerate(sizes)]
    per_row = [(n + 127) // 128 - (i + 1) // 128 for _, n in jobs for i in range(n - 1)]   # chunks of every row with a j > i
    starts = np.concatenate([[0], np.cumsum(per_row)])
    first = np.arange(0, starts[-1], 8)                                                    # every workgroup's first chunk
    assert len(per_row) > 4096 and {1, 2, 3} == set(per_row)
    assert starts[-1] % 8 != 0 and np.isin(first, starts, invert=True).mean() > 0.5
    want = np.concatenate([table[ids[r0:r0 + n][i], ids[r0:r0 + n][j]] for r0, n in jobs for i, j in [np.triu_indices(n, 1)]])
    assert (want >= 0).sum() > 50000 and (want == -1).sum() > 50000
    rc, got, _ = pairs_raw([pool[x] for x in ids], [kpool[x] for x in ids], jobs)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    bad = np.nonzero(got != want)[0]
    assert got.size == want.size > 500000 and bad.size == 0, \
        f"{bad.size} of {got.size} distances differ: {[(int(x), int(got[x]), int(want[x])) for x in bad[:10]]}"


def neighbour_matrix(dist, n):
    """The host reduction of a job's distances: n x ceil(n / 32) words, bit j of row i = the pair is within its limit."""
    nw = (n + 31) // 32
    adj = np.zeros((n, nw), dtype=np.uint32)
    x = 0
    for i in range(n):
        for j in range(i + 1, n):
            if dist[x] >= 0:
                adj[i, j // 32] |= np.uint32(1 << (j % 32))
                adj[j, i // 32] |= np.uint32(1 << (i % 32))
            x += 1
    return adj


@pytest.fixture(scope="module")
def families():
    """Jobs of n = 0, 1, 2, 31, 32, 33, 64, 127, 128, 129, 130 reads of 150-260 nt (3-5 words), each job two or three
    families of mutated copies plus unrelated reads, so that both bit values are common."""
    rng = random.Random(33)
    reads, ks, jobs = [], [], []
    for n in (1, 2, 31, 0, 32, 33, 64, 127, 128, 129, 130):
        bases = [rand_seq(rng, rng.randrange(170, 240)) for _ in range(3)]
        jobs.append((len(reads), n))
        for _ in range(n):
            r = mutate(rng, rng.choice(bases), rng.uniform(0.0, 0.12)) if rng.random() < 0.8 else \
                rand_seq(rng, rng.randrange(150, 261))
            r = r[:260].ljust(150, "A")
            reads.append(r)
            ks.append(int(len(r) * (1 - 0.9)))
    return reads, ks, jobs


def test_neighbours_equal_the_reduced_distances(families):
    reads, ks, jobs = families
    assert all(150 <= len(r) <= 260 for r in reads)
    rc, dist, _ = pairs_raw(reads, ks, jobs)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    rc, adj, ms = pairs_raw(reads, ks, jobs, neighbours=True)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert ms > 0
    at_d = at_a = 0
    ones = 0
    for r0, n in jobs:
        if n == 0:
            continue
        nd, nw = n * (n - 1) // 2, (n + 31) // 32
        got = adj[at_a:at_a + n * nw].reshape(n, nw)
        want = neighbour_matrix(dist[at_d:at_d + nd], n)
        assert np.array_equal(got, want), (n, np.argwhere(got != want)[:5])   # word for word
        bits = np.unpackbits(got.view(np.uint8), axis=1, bitorder="little")
        assert not bits[:, n:].any()                                          # zero padding bits
        sq = bits[:, :n]
        assert np.array_equal(sq, sq.T) and not sq.diagonal().any()           # symmetric, zero diagonal
        ones += int(sq.sum())
        at_d += nd
        at_a += n * nw
    assert at_d == dist.size and at_a == adj.size
    assert 0.05 < ones / (2 * dist.size) < 0.95
    # a sample of 500 pairs against the oracle
    pairs = job_pairs(jobs)
    rng = random.Random(34)
    for x in rng.sample(range(len(pairs)), 500):
        i, j = pairs[x]
        assert dist[x] == oracle_dist(reads[i], reads[j], pair_limit(ks[i], ks[j])), (i, j)


def test_second_call_reuses_the_workspace(families):
    reads, ks, jobs = families
    rng = random.Random(35)
    first = pairs_raw(reads, ks, jobs, neighbours=True)
    small_reads = [rand_seq(rng, 40), rand_seq(rng, 40), "ACGTACGT", "ACGAACGT", rand_seq(rng, 1300)]
    small_reads.append(mutate(rng, small_reads[-1], 0.03))
    small_ks = [4, 4, 1, 1, 130, 130]
    small_jobs = [(0, 2), (2, 2), (4, 2)]
    for sentinel in (-7, 123456):
        rc, got, _ = pairs_raw(small_reads, small_ks, small_jobs, sentinel=sentinel)
        assert rc == _lib.OK and np.array_equal(got, expected_dists(small_reads, small_ks, small_jobs))
    for sentinel in (0, 0xFFFFFFFF):
        rc, got, _ = pairs_raw(small_reads, small_ks, small_jobs, neighbours=True, sentinel=sentinel)
        assert rc == _lib.OK and got.tolist() == [0, 0, 2, 1, 2, 1]           # only the last two pairs are neighbours
        again = pairs_raw(reads, ks, jobs, neighbours=True, sentinel=sentinel)
        assert again[0] == _lib.OK and np.array_equal(again[1], first[1])
    rc, got, _ = pairs_raw(["ACGT"], [1], [(0, 1), (0, 0)], neighbours=True)  # jobs of one and of no read only
    assert rc == _lib.OK and got.tolist() == [0]
    rc, got, _ = pairs_raw(["ACGT"], [1], [])
    assert rc == _lib.OK and got.size == 0


def lds_table_bytes(m, rows):
    """LDS bytes of a read's Peq table: MINE_LDS_HEAD words + (rows + 1) x (W | 1) words, as in specimine."""
    return (192 + (rows + 1) * (((m + 63) // 64) | 1)) * 8


def all_bytes_read(rng, m):
    q = list(ALL_BYTES) + [rng.choice(ALL_BYTES) for _ in range(m - 256)]
    rng.shuffle(q)
    return "".join(q)


def test_lds_limit_at_its_edge():
    """SMX_LDS_POOL = 159744 bytes: 256 distinct bytes fit at m = 4800 (W = 75) and not at m = 4864 (W = 76, Wp = 77)."""
    rng = random.Random(36)
    fits, over = all_bytes_read(rng, 4800), all_bytes_read(rng, 4864)
    assert lds_table_bytes(4800, 256) == 155736 <= 159744 < lds_table_bytes(4864, 256) == 159848
    t = mutate(rng, fits, 0.04, ALL_BYTES)
    d = oracle_dist(fits, t, -1)
    for k in (-1, d, d - 1):
        assert_dists([fits, t], [k, k], [(0, 2)])
    rc, _, _ = pairs_raw([over, mutate(rng, over, 0.04, ALL_BYTES)[:4000]], [-1, -1], [(0, 2)])
    msg = _lib.load().smx_last_error().decode()
    assert rc == _lib.ERR_UNSUPPORTED and "do not fit the LDS" in msg and "159848 > 159744" in msg, (rc, msg)
    assert_dists([fits[:700], t[:760], fits[:3000]], [100, 100, -1], [(0, 3)])   # the next call is unaffected


def test_overlapping_and_out_of_range_jobs_are_rejected():
    rng = random.Random(37)
    reads = [rand_seq(rng, 50) for _ in range(6)]
    ks = [5] * 6
    lib = _lib.load()
    for neighbours in (False, True):
        rc, _, _ = pairs_raw(reads, ks, [(0, 4), (3, 3)], neighbours=neighbours)
        assert rc == _lib.ERR_ARG and "overlap" in lib.smx_last_error().decode()
        rc, _, _ = pairs_raw(reads, ks, [(3, 3), (1, 0), (0, 4)], neighbours=neighbours)
        assert rc == _lib.ERR_ARG and "overlap" in lib.smx_last_error().decode()
        rc, _, _ = pairs_raw(reads, ks, [(4, 3)], neighbours=neighbours)
        assert rc == _lib.ERR_ARG and "out of bounds" in lib.smx_last_error().decode()
        rc, _, _ = pairs_raw(reads, ks, [(3, 3), (2, 0), (0, 3)], neighbours=neighbours)   # touching, an empty job inside
        assert rc == _lib.OK
    assert_dists(reads, ks, [(3, 3), (0, 3)])
