"""The two launch-geometry branches of the chunked long-read kernels that the other GPU tests never reach, with sequences of
a few bases so that each call takes little more than its launches:

  * chunk_owner's fourth round (smx_mine_lds.h): more than 262 144 records in one launch, on the specimine kernel (one
    record per (job, query)), the clusters kernel (one per row) and the consensus kernel (one per job);
  * the stride over the jobs behind the 65 535 cap of gridDim.y / gridDim.x in cons_vote_kernel, phase_sites_kernel,
    phase_planes_kernel and phase_link_kernel: one smx_cons_phase call over more than 65 535 jobs.

Every reference is built by aligning each distinct pair (or job) of a small pool once with the suite's plain twins, then
gathered with numpy; every output element of every call is compared with ==.  Each test prints the call's kernel time."""
import random
import time

import numpy as np
import pytest

from clusters_utils import mutate, rand_seq
from oracle.edlib_semantics import HW, NW, align_c
from specimux_amd import _lib, calls
from variants_utils import phase_reference

pytestmark = pytest.mark.gpu

OWNER_ROUND_4 = 64 ** 3 + 1            # records from which the 64-way search takes a fourth round
GRID_DIM_CAP = 65535


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def within_groups(counts):
    """(group of every element, its index within the group) for groups of the given sizes laid end to end."""
    counts = np.asarray(counts, dtype=np.int64)
    group = np.repeat(np.arange(counts.size), counts)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return group, np.arange(counts.sum()) - start[group]


def differing(got, want):
    bad = np.nonzero(got != want)[0]
    return f"{bad.size} of {got.size} differ: {[(int(x), got[x], want[x]) for x in bad[:10]]}"


# ---------------------------------------------------------------------------------------------------- specimine
@pytest.fixture(scope="module")
def mine_records():
    """More than 262 144 (job, query) records in state class 1: 48 queries and 64 target strings of at most 16 bases, 700
    targets drawn from the strings, one job per record over 1, 2 or 129 of the targets (one or two chunks)."""
    rng = random.Random(141)
    qpool = [rand_seq(rng, 1 + i % 16) for i in range(48)]
    kpool = [rng.choice((-1, 0, 1, 3)) for _ in qpool]
    tpool = [(mutate(rng, qpool[i % 48], 0.2) or "A")[:16] if i % 2 else rand_seq(rng, 1 + (i * 5) % 16) for i in range(64)]
    table = np.array([[align_c(q, t, HW, k, iupac=False)["editDistance"] for t in tpool] for q, k in zip(qpool, kpool)], dtype=np.int64)
    n_rec = OWNER_ROUND_4 + 355
    r = np.random.default_rng(142)
    qid = r.integers(0, 48, n_rec)
    tid = r.integers(0, 64, 700)
    nt = np.where(np.arange(n_rec) % 16 == 7, 129, np.where(np.arange(n_rec) % 16 == 3, 2, 1))
    t0 = r.integers(0, 700 - 129, n_rec)
    min_identity = np.array([0.0, 0.9, 0.5])[np.arange(n_rec) % 3]
    jobs = np.zeros(n_rec, dtype=_lib.MINE_JOB_DTYPE)
    jobs["q0"], jobs["nq"], jobs["t0"], jobs["nt"], jobs["min_identity"] = qid, 1, t0, nt, min_identity
    # the launch walks the records in query order (a stable sort): some records own two chunks, some workgroups of 8
    # chunks start inside one, and the chunk total is no multiple of 8
    order = np.argsort(qid, kind="stable")
    starts = np.concatenate([[0], np.cumsum((nt[order] + 127) // 128)])
    first = np.arange(0, starts[-1], 8)
    assert n_rec > 262144 and set(np.diff(starts)) == {1, 2}
    assert starts[-1] % 8 != 0 and np.isin(first, starts, invert=True).mean() > 0.02
    rec, i = within_groups(nt)
    want = table[qid[rec], tid[t0[rec] + i]]
    assert (want >= 0).sum() > 100000 and (want == -1).sum() > 100000
    qlen = np.array([len(q) for q in qpool])
    with np.errstate(invalid="ignore"):
        identity = np.where(want < 0, 0.0, 1.0 - want.astype(np.float64) / qlen[qid[rec]].astype(np.float64))
    best = np.where((identity >= min_identity[rec]) & (identity > 0.0), identity, 0.0)
    assert (best > 0).sum() > 50000 and ((identity > 0) & (best == 0)).sum() > 10000
    args = dict(queries="".join(qpool).encode(), qoff=offsets(qlen), ks=np.array(kpool, dtype=np.int32),
                targets="".join(tpool[x] for x in tid).encode(), toff=offsets([len(tpool[x]) for x in tid]), jobs=jobs)
    return args, want, best


def mine_call(args, best):
    lib = _lib.load()
    n_out = int(args["jobs"]["nt"].sum())          # one query per job: both modes have sum(nt) outputs
    out = np.full(n_out, -5.0, dtype=np.float64) if best else np.full(n_out, -7, dtype=np.int32)
    ms = []
    t = time.perf_counter()
    rc = calls.invoke("smx_mine_best_identity" if best else "smx_mine_distances", args["queries"], _lib.ptr(args["qoff"]), 48,
                      _lib.ptr(args["ks"]), args["targets"], _lib.ptr(args["toff"]), 700, _lib.ptr(args["jobs"]), len(args["jobs"]),
                      _lib.ptr(out), kernel_ms=ms, check=False)
    assert rc == _lib.OK, lib.smx_last_error()
    print(f"\nsmx_mine_{'best_identity' if best else 'distances'}: {len(args['jobs'])} records, {n_out} outputs, "
          f"kernel {ms[0]:.2f} ms, call {time.perf_counter() - t:.2f} s")
    return out


def test_specimine_distances_over_262144_records(mine_records):
    args, want, _best = mine_records
    got = mine_call(args, best=False)
    assert got.size == want.size > 2_000_000 and np.array_equal(got, want), differing(got, want)


def test_specimine_best_identity_over_262144_records(mine_records):
    args, _want, best = mine_records
    got = mine_call(args, best=True)
    assert got.size == best.size and np.array_equal(got, best), differing(got, best)


# ----------------------------------------------------------------------------------------------------- clusters
def nw_dist(a, b, k):
    d = align_c(a, b, NW, k, iupac=False)["editDistance"]
    return -1 if (not a or not b) and 0 <= k < d else d


@pytest.fixture(scope="module")
def pairs_rows():
    """More than 262 144 rows in state class 1: 131 100 jobs of three reads (two rows each), then one job of 129 reads
    whose first row owns two chunks; the reads are 48 strings of at most 16 bases."""
    rng = random.Random(143)
    pool = [rand_seq(rng, 1 + i % 16) for i in range(24)]
    pool += [(mutate(rng, p, 0.15) or p)[:16] for p in pool]
    kpool = [rng.choice((-1, 1, 2, 5)) for _ in pool]
    limit = lambda ka, kb: -1 if ka < 0 or kb < 0 else max(ka, kb)
    table = np.array([[nw_dist(a, b, limit(ka, kb)) for b, kb in zip(pool, kpool)] for a, ka in zip(pool, kpool)], dtype=np.int64)
    n3 = 131100
    r = np.random.default_rng(144)
    ids = r.integers(0, 48, 3 * n3 + 129)
    jobs = np.zeros(n3 + 1, dtype=_lib.PAIRS_JOB_DTYPE)
    jobs["r0"], jobs["n"] = 3 * np.arange(n3 + 1), 3
    jobs["n"][-1] = 129
    assert 2 * n3 + 128 > 262144
    a, b, c = ids[0:3 * n3:3], ids[1:3 * n3:3], ids[2:3 * n3:3]
    big = ids[3 * n3:]
    bi, bj = np.triu_indices(129, 1)
    dist = np.concatenate([np.stack([table[a, b], table[a, c], table[b, c]], axis=1).ravel(), table[big[bi], big[bj]]])
    assert (dist >= 0).sum() > 100000 and (dist == -1).sum() > 100000
    # adjacency: a job of three has one word per row; the job of 129 has five words per row, mirrored
    ab, ac, bc = (table[x, y] >= 0 for x, y in ((a, b), (a, c), (b, c)))
    small = np.stack([ab * 2 + ac * 4, ab * 1 + bc * 4, ac * 1 + bc * 2], axis=1).astype(np.uint32).ravel()
    near = np.zeros((129, 129), dtype=bool)
    near[bi, bj] = table[big[bi], big[bj]] >= 0
    near |= near.T
    bits = np.zeros((129, 160), dtype=np.uint64)
    bits[:, :129] = near
    words = (bits.reshape(129, 5, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    adj = np.concatenate([small, words.ravel()])
    reads = [pool[x].encode() for x in ids]
    args = dict(reads=b"".join(reads), roff=offsets([len(x) for x in reads]), n_reads=len(reads),
                ks=np.array([kpool[x] for x in ids], dtype=np.int32), jobs=jobs)
    return args, dist, adj


def pairs_call(args, n_out, neighbours):
    lib = _lib.load()
    out = np.full(n_out, 0xDEADBEEF, dtype=np.uint32) if neighbours else np.full(n_out, -7, dtype=np.int32)
    ms = []
    t = time.perf_counter()
    rc = calls.invoke("smx_pairs_neighbours" if neighbours else "smx_pairs_distances", args["reads"], _lib.ptr(args["roff"]),
                      args["n_reads"], _lib.ptr(args["ks"]), _lib.ptr(args["jobs"]), len(args["jobs"]), _lib.ptr(out), kernel_ms=ms,
                      check=False)
    assert rc == _lib.OK, lib.smx_last_error()
    print(f"\nsmx_pairs_{'neighbours' if neighbours else 'distances'}: {len(args['jobs'])} jobs, {n_out} outputs, "
          f"kernel {ms[0]:.2f} ms, call {time.perf_counter() - t:.2f} s")
    return out


def test_clusters_distances_over_262144_rows(pairs_rows):
    args, dist, _adj = pairs_rows
    got = pairs_call(args, dist.size, neighbours=False)
    assert np.array_equal(got, dist), differing(got, dist)


def test_clusters_neighbours_over_262144_rows(pairs_rows):
    args, _dist, adj = pairs_rows
    got = pairs_call(args, adj.size, neighbours=True)
    assert np.array_equal(got, adj), differing(got, adj)


# ------------------------------------------------------------------------------- consensus votes and the variant kernels
def test_cons_phase_over_65535_jobs():
    """One smx_cons_phase call over more than 65 535 jobs of two members around 8-nt drafts, max_sites = 2: votes, aligned,
    sites, planes and link tables of every job against phase_reference over the 64 distinct (draft, other member) pairs of
    a pool of eight reads.  cons_vote_kernel and the three phase kernels stride over the jobs behind their grid cap."""
    rng = random.Random(145)
    q = rand_seq(rng, 8)
    sub = lambda s, edits: "".join("ACGT"[("ACGT".index(c) + edits[p]) % 4] if p in edits else c for p, c in enumerate(s))
    pool = [q, q, sub(q, {2: 1}), sub(q, {5: 2}), sub(q, {1: 1, 6: 3}), sub(q, {0: 1, 3: 1, 7: 2}), q[:4] + q[5:] + "A", rand_seq(rng, 8)]
    pool = [p.encode() for p in pool]
    assert all(len(p) == 8 for p in pool)
    max_sites, min_permille, min_reads, k = 2, 150, 1, 3
    # the twin over every (draft = first member, second member) pair of the pool
    combos = [(a, b) for a in range(8) for b in range(8)]
    ref = phase_reference([pool[x] for ab in combos for x in ab], [k] * 128, [(2 * c, 2 * c, 2) for c in range(64)],
                          min_permille, min_reads, max_sites)
    ref_votes = np.stack([np.asarray(w.table, dtype=np.uint32).reshape(9, 26) for w in ref])
    ref_aligned = np.array([w.aligned for w in ref], dtype=np.uint32)
    ref_sites = np.zeros((64, max_sites), dtype=_lib.CONS_SITE_DTYPE)          # the slots past the kept sites are zero
    for c, w in enumerate(ref):
        for s, site in enumerate(w.sites):
            ref_sites[c, s] = (site.pos, site.kind, site.major, site.minor, 0, site.n_major, site.n_minor)
    ref_n_sites = np.array([len(w.sites) for w in ref], dtype=np.uint32)
    ref_n_qualified = np.array([w.n_qualified for w in ref], dtype=np.uint32)
    ref_planes = np.stack([np.asarray(w.planes, dtype=np.uint64).reshape(max_sites, 2, 1) for w in ref])
    ref_link = np.stack([np.asarray(w.link, dtype=np.uint32) for w in ref])
    assert set(ref_n_sites) == {0, 1, 2} and (ref_n_qualified > max_sites).any() and (ref_aligned < 2).any()
    n_jobs = GRID_DIM_CAP + 166
    r = np.random.default_rng(146)
    combo = r.integers(0, 64, n_jobs)
    combo[-3] = combos.index((0, 4))                                            # near the end: a second allele at two sites
    assert ref_n_sites[combo[-3]] == 2 and ref_link[combo[-3]].any()
    ids = np.array(combos)[combo].ravel()
    reads = [pool[x] for x in ids]
    jobs = np.zeros(n_jobs, dtype=_lib.CONS_JOB_DTYPE)
    jobs["draft"] = jobs["r0"] = 2 * np.arange(n_jobs)
    jobs["n"] = 2
    votes = np.full((n_jobs, 9, 26), 0xDEADBEEF, dtype=np.uint32)
    aligned = np.full(n_jobs, 0xDEADBEEF, dtype=np.uint32)
    sites = np.frombuffer(np.full(n_jobs * max_sites * 4, 0xDEADBEEF, dtype=np.uint32).tobytes(), dtype=_lib.CONS_SITE_DTYPE).copy()
    n_sites = np.full(n_jobs, 0xDEADBEEF, dtype=np.uint32)
    n_qualified = np.full(n_jobs, 0xDEADBEEF, dtype=np.uint32)
    planes = np.full((n_jobs, max_sites, 2, 1), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    link = np.full((n_jobs, max_sites, max_sites, 4), 0xDEADBEEF, dtype=np.uint32)
    lib = _lib.load()
    ms = []
    t = time.perf_counter()
    rc = calls.invoke("smx_cons_phase", b"".join(reads), _lib.ptr(offsets([8] * len(reads))), len(reads),
                      _lib.ptr(np.full(len(reads), k, dtype=np.int32)), _lib.ptr(jobs), n_jobs, min_permille, min_reads, max_sites,
                      _lib.ptr(votes), _lib.ptr(aligned), _lib.ptr(sites), _lib.ptr(n_sites), _lib.ptr(n_qualified), _lib.ptr(planes),
                      _lib.ptr(link), kernel_ms=ms, check=False)
    assert rc == _lib.OK, lib.smx_last_error()
    print(f"\nsmx_cons_phase: {n_jobs} jobs, kernel {ms[0]:.2f} ms, call {time.perf_counter() - t:.2f} s")
    assert n_jobs > GRID_DIM_CAP
    assert np.array_equal(aligned, ref_aligned[combo]), differing(aligned, ref_aligned[combo])
    assert np.array_equal(votes, ref_votes[combo]), np.argwhere(votes != ref_votes[combo])[:5]
    assert np.array_equal(n_sites, ref_n_sites[combo]), differing(n_sites, ref_n_sites[combo])
    assert np.array_equal(n_qualified, ref_n_qualified[combo]), differing(n_qualified, ref_n_qualified[combo])
    want_sites = ref_sites[combo].ravel()
    for field in ("pos", "kind", "major", "minor", "n_major", "n_minor"):       # kept sites, and zeros in the slots past them
        assert np.array_equal(sites[field], want_sites[field]), (field, differing(sites[field], want_sites[field]))
    assert np.array_equal(planes, ref_planes[combo]), np.argwhere(planes != ref_planes[combo])[:5]
    assert np.array_equal(link, ref_link[combo]), np.argwhere(link != ref_link[combo])[:5]
