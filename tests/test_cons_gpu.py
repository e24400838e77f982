"""The consensus kernels on the GPU (smx_cons.hip through smx_cons_pileup / smx_cons_votes): distances and pileup rows
word for word against the full-matrix twin (cons_utils.row_reference), the vote tables against a numpy reduction of
those rows, and the limits of the call."""
import random
import re

import numpy as np
import pytest

from clusters_utils import mutate, rand_seq
from cons_utils import NO_ROW, pileup_reference, reduce_rows, row_reference
from specimux_amd import _lib, calls

pytestmark = pytest.mark.gpu

ALL_BYTES = "".join(map(chr, range(256)))


def cons_raw(reads, ks, jobs, votes=False):
    """One smx_cons_pileup / smx_cons_votes call on bytes reads; jobs are (draft, r0, n).  The outputs are filled with
    a sentinel first.  -> (status, rows or votes, dist or aligned, kernel ms)."""
    roff = calls.offsets(reads)
    jobs = [tuple(j) for j in jobs]
    words = [len(reads[d]) + 1 if d < len(reads) else 0 for d, _, _ in jobs]
    jarr = calls.job_array(jobs, _lib.CONS_JOB_DTYPE)
    if votes:
        n_a, n_b = sum(w * 26 for w in words), len(jobs)
        b = np.full(max(n_b, 1), 0xDEADBEEF, dtype=np.uint32)
        fn = "smx_cons_votes"
    else:
        n_a, n_b = sum(w * n for w, (_, _, n) in zip(words, jobs)), sum(n for _, _, n in jobs)
        b = np.full(max(n_b, 1), -7, dtype=np.int32)
        fn = "smx_cons_pileup"
    a = np.full(max(n_a, 1), 0xDEADBEEF, dtype=np.uint32)
    ms = []
    rc = calls.invoke(fn, b"".join(reads), _lib.ptr(roff), len(reads), _lib.ptr(np.array(ks, dtype=np.int32)), _lib.ptr(jarr),
                      len(jobs), _lib.ptr(a), _lib.ptr(b), kernel_ms=ms, check=False)
    return rc, a[:n_a], b[:n_b], ms[0]


def member_set(rng, q, kd, alphabet):
    """The draft's members with their own limits: the draft itself, point edits, 1- and 6-base insertions and
    deletions at the start, on a block row in the middle and at the end, a read exactly at its limit and the same read
    one above it, an empty read within and one above its limit, and an unrelated read without a limit."""
    m = len(q)
    mid = (m // 2) & ~63 if m > 64 else m // 2               # a block row (a multiple of 64) where the draft has one
    out = [(q, kd), (mutate(rng, q, 0.03, alphabet), kd), (mutate(rng, q, 0.06, alphabet), kd)]
    for at in (0, mid, m):
        for size in (1, 6):
            out.append((q[:at] + rand_seq(rng, size, alphabet) + q[at:], kd))
            cut = min(at, max(m - size, 0))
            out.append((q[:cut] + q[cut + size:], kd))
    far = mutate(rng, q, 0.25, alphabet) + rand_seq(rng, 3, alphabet)
    d, _ = row_reference(q.encode("latin-1"), far.encode("latin-1"), -1)
    if d - 1 >= kd:                                           # the pair's limit is max(kd, the member's): d, then d - 1
        out += [(far, d), (far, d - 1)]
    out += [("", m), ("", 0), (rand_seq(rng, m + rng.randrange(0, 40), alphabet), -1)]
    return out


@pytest.fixture(scope="module")
def shapes():
    """One call: per draft length and alphabet a job over member_set (two jobs per register class: the two alphabets;
    jobs of different classes side by side), then jobs of 1, 127, 128 and 129 members around short drafts, a job whose
    draft is not one of its members and one without members.  With the twin's rows and distances."""
    rng = random.Random(61)
    reads, ks, jobs = [], [], []
    for m in (1, 63, 64, 65, 129, 257, 600, 1030):
        for alphabet in ("ACGT", "ACGTN"):
            q = rand_seq(rng, m, alphabet)
            members = member_set(rng, q, m // 10, alphabet)
            jobs.append((len(reads), len(reads), len(members)))
            reads += [r for r, _ in members]
            ks += [k for _, k in members]
    for n in (1, 127, 128, 129):
        q = rand_seq(rng, rng.randrange(60, 70), "ACGTN")
        jobs.append((len(reads), len(reads), n))
        reads += [q] + [mutate(rng, q, rng.uniform(0.0, 0.2), "ACGTN") for _ in range(n - 1)]
        ks += [6] * n
    outside = len(reads)
    reads.append(rand_seq(rng, 200))
    ks.append(20)
    jobs.append((outside, len(reads), 5))                     # the draft is not a member
    reads += [mutate(rng, reads[outside], 0.04) for _ in range(5)]
    ks += [20] * 5
    jobs.append((outside, len(reads), 0))                     # no members
    raw = [r.encode("latin-1") for r in reads]
    rows, dist = pileup_reference(raw, ks, jobs)
    return raw, ks, jobs, rows, dist


def test_pileup_equals_the_reference(shapes):
    reads, ks, jobs, want_rows, want_dist = shapes
    rc, rows, dist, ms = cons_raw(reads, ks, jobs)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert ms > 0
    assert (want_dist >= 0).sum() > 400 and (want_dist == -1).sum() > 40 and (want_dist == 0).sum() >= 20
    bad = np.nonzero(dist != want_dist)[0]
    assert bad.size == 0, [(int(x), int(dist[x]), int(want_dist[x])) for x in bad[:10]]
    at = 0
    for draft, r0, n in jobs:                                  # row by row, to name the first one that differs
        words = len(reads[draft]) + 1
        for i in range(n):
            got, want = rows[at:at + words], want_rows[at:at + words]
            if not np.array_equal(got, want):
                p = int(np.nonzero(got != want)[0][0])
                raise AssertionError(f"draft of {words - 1}, member {i} of {n} (length {len(reads[r0 + i])}), word {p}: "
                                     f"{int(got[p]):#x} != {int(want[p]):#x}")
            at += words
    assert at == rows.size == want_rows.size
    assert (want_rows == NO_ROW).any() and ((want_rows >> 3) & 255 >= 6).any() and ((want_rows & 7) == 4).any()


def test_pileup_walk_over_many_short_jobs(monkeypatch):
    """The chunk walk (smx_mine_lds.h) where it can go wrong, all in state class 1: more than 4096 jobs, so that the owner
    search takes its third round, of 1, 2 and 129 members in turn, so that a job of 129 owns two chunks.  Once with one
    chunk per workgroup, and once with a history workspace of 39 slices: 39 workgroups of ceil(chunks / 39) chunks,
    some of which start inside a job and the last of which is short.  The reads are drawn from a small pool, so the
    twin aligns every distinct pair once; every distance and every row word of both calls is compared."""
    rng = random.Random(63)
    pool = [rand_seq(rng, rng.randrange(12, 41)) for _ in range(20)]
    pool += [(mutate(rng, r, 0.1) or r)[:40].ljust(12, "A") for r in pool]
    pool = [r.encode("latin-1") for r in pool]
    kpool = [rng.choice((-1, 3, 6, 12)) for _ in pool]
    twin = {}
    for a in range(len(pool)):
        for b in range(len(pool)):
            d, row = row_reference(pool[a], pool[b], -1 if kpool[a] < 0 or kpool[b] < 0 else max(kpool[a], kpool[b]))
            twin[a, b] = d, np.array(row, dtype=np.uint32)
    sizes = [(1, 2, 129)[j % 3] for j in range(4099)]
    ids = [rng.randrange(len(pool)) for _ in range(sum(sizes))]
    jobs, r0 = [], 0
    for n in sizes:
        jobs.append((r0 + rng.randrange(n), r0, n))            # the draft: one of the job's own members
        r0 += n
    want_dist = np.array([twin[ids[d], ids[r]][0] for d, r0, n in jobs for r in range(r0, r0 + n)], dtype=np.int32)
    want_rows = np.concatenate([twin[ids[d], ids[r]][1] for d, r0, n in jobs for r in range(r0, r0 + n)])
    assert (want_dist >= 0).sum() > 20000 and (want_dist == -1).sum() > 20000
    chunks = sum((n + 127) // 128 for n in sizes)
    starts = np.concatenate([[0], np.cumsum([(n + 127) // 128 for n in sizes])])
    per_block = -(-chunks // 39)
    first = np.arange(0, chunks, per_block)                     # every workgroup's first chunk in the second call
    assert chunks % per_block != 0 and np.isin(first, starts, invert=True).sum() >= 5
    reads, ks = [pool[x] for x in ids], [kpool[x] for x in ids]
    monkeypatch.setenv("SMX_CONS_HIST_BYTES", "1")
    assert cons_raw(reads, ks, jobs)[0] == _lib.ERR_UNSUPPORTED
    need = int(re.search(r"needs (\d+) bytes", _lib.load().smx_last_error().decode()).group(1))
    for budget in (None, 39 * need):
        if budget is None:
            monkeypatch.delenv("SMX_CONS_HIST_BYTES")
        else:
            monkeypatch.setenv("SMX_CONS_HIST_BYTES", str(budget))
        rc, rows, dist, _ms = cons_raw(reads, ks, jobs)
        assert rc == _lib.OK, _lib.load().smx_last_error()
        bad = np.nonzero(dist != want_dist)[0]
        assert bad.size == 0, (budget, bad.size, [(int(x), int(dist[x]), int(want_dist[x])) for x in bad[:10]])
        bad = np.nonzero(rows != want_rows)[0]
        assert rows.size == want_rows.size and bad.size == 0, (budget, bad.size, bad[:10].tolist())


def test_votes_equal_the_reduced_rows(shapes):
    reads, ks, jobs, want_rows, want_dist = shapes
    rc, votes, aligned, ms = cons_raw(reads, ks, jobs, votes=True)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert ms > 0
    at_r = at_d = at_v = 0
    for j, (draft, r0, n) in enumerate(jobs):
        m = len(reads[draft])
        rows = want_rows[at_r:at_r + n * (m + 1)].reshape(n, m + 1)
        ok = want_dist[at_d:at_d + n] >= 0
        want = reduce_rows(rows[ok], m)
        got = votes[at_v:at_v + (m + 1) * 26].reshape(m + 1, 26)
        assert np.array_equal(got, want), (j, m, n, np.argwhere(got != want)[:5])
        assert aligned[j] == ok.sum()
        at_r, at_d, at_v = at_r + n * (m + 1), at_d + n, at_v + (m + 1) * 26
    assert at_v == votes.size
    assert aligned[-1] == 0 and not votes[-201 * 26:].any()    # the job without members: a zero table
    again = cons_raw(reads, ks, jobs, votes=True)
    assert np.array_equal(again[1], votes) and np.array_equal(again[2], aligned)   # no atomics: the same from run to run


def test_second_call_reuses_the_workspace(shapes):
    reads, ks, jobs, want_rows, want_dist = shapes
    rng = random.Random(62)
    q = rand_seq(rng, 40)
    small = [q.encode(), mutate(rng, q, 0.1).encode(), b"ACGTACGT", b"ACGAACG"]
    small_ks, small_jobs = [6, 6, 2, 2], [(0, 0, 2), (2, 2, 2)]
    want = pileup_reference(small, small_ks, small_jobs)
    for _ in range(2):
        rc, rows, dist, _ms = cons_raw(small, small_ks, small_jobs)
        assert rc == _lib.OK and np.array_equal(rows, want[0]) and np.array_equal(dist, want[1])
        rc, rows, dist, _ms = cons_raw(reads, ks, jobs)
        assert rc == _lib.OK and np.array_equal(rows, want_rows) and np.array_equal(dist, want_dist)
    rc, rows, dist, _ms = cons_raw(small, small_ks, [])
    assert rc == _lib.OK and rows.size == 0 and dist.size == 0


def test_few_workgroups_in_flight(shapes, monkeypatch):
    """A history workspace of one slice: every class runs as one workgroup over all of its chunks, the Peq table rebuilt
    from job to job; one byte less is refused before anything runs."""
    reads, ks, jobs, want_rows, want_dist = shapes
    monkeypatch.setenv("SMX_CONS_HIST_BYTES", "1")
    rc, _, _, _ = cons_raw(reads, ks, jobs)
    msg = _lib.load().smx_last_error().decode()
    assert rc == _lib.ERR_UNSUPPORTED and "history" in msg, (rc, msg)
    need = int(re.search(r"needs (\d+) bytes", msg).group(1))
    monkeypatch.setenv("SMX_CONS_HIST_BYTES", str(need - 1))
    assert cons_raw(reads, ks, jobs)[0] == _lib.ERR_UNSUPPORTED
    monkeypatch.setenv("SMX_CONS_HIST_BYTES", str(need))
    rc, rows, dist, _ms = cons_raw(reads, ks, jobs)
    assert rc == _lib.OK and np.array_equal(rows, want_rows) and np.array_equal(dist, want_dist)


def lds_table_bytes(m, rows):
    return (192 + (rows + 1) * (((m + 63) // 64) | 1)) * 8


def all_bytes_read(rng, m):
    q = list(ALL_BYTES) + [rng.choice(ALL_BYTES) for _ in range(m - 256)]
    rng.shuffle(q)
    return "".join(q)


def test_lds_limit_at_its_edge():
    """SMX_LDS_POOL = 159744 bytes: a draft of 256 distinct bytes fits at m = 4800 (W = 75) and not at m = 4864."""
    rng = random.Random(63)
    fits, over = all_bytes_read(rng, 4800), all_bytes_read(rng, 4864)
    assert lds_table_bytes(4800, 256) == 155736 <= 159744 < lds_table_bytes(4864, 256) == 159848
    t = mutate(rng, fits, 0.04, ALL_BYTES)
    reads = [fits.encode("latin-1"), t.encode("latin-1"), t.encode("latin-1")]
    d, row = row_reference(reads[0], reads[1], -1)
    ks = [d - 1, d, d - 1]                                    # the pair limits d and d - 1
    rc, rows, dist, _ms = cons_raw(reads, ks, [(0, 1, 2)])
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert dist.tolist() == [d, -1]
    assert np.array_equal(rows[:4801], np.array(row, dtype=np.uint32)) and (rows[4801:] == NO_ROW).all()
    bad = [over.encode("latin-1"), mutate(rng, over, 0.04, ALL_BYTES)[:4000].encode("latin-1")]
    for votes in (False, True):
        rc, _, _, _ = cons_raw(bad, [400, 400], [(0, 1, 1)], votes=votes)
        msg = _lib.load().smx_last_error().decode()
        assert rc == _lib.ERR_UNSUPPORTED and "do not fit the LDS" in msg and "159848 > 159744" in msg, (rc, msg)
    small = [b"ACGTACGT", b"ACGAACG"]                          # the next call is unaffected
    rc, rows, dist, _ms = cons_raw(small, [2, 2], [(0, 0, 2)])
    want = pileup_reference(small, [2, 2], [(0, 0, 2)])
    assert rc == _lib.OK and np.array_equal(rows, want[0]) and np.array_equal(dist, want[1])


def test_bad_jobs_are_rejected():
    """Host checks only: nothing is launched for a call that is refused."""
    rng = random.Random(64)
    reads = [rand_seq(rng, 50).encode() for _ in range(6)] + [b""]
    ks = [5] * 7
    lib = _lib.load()
    for votes in (False, True):
        rc, _, _, _ = cons_raw(reads, ks, [(6, 0, 3)], votes=votes)
        assert rc == _lib.ERR_ARG and "empty draft" in lib.smx_last_error().decode()
        rc, _, _, _ = cons_raw(reads, ks, [(0, 0, 4), (1, 3, 3)], votes=votes)
        assert rc == _lib.ERR_ARG and "overlap" in lib.smx_last_error().decode()
        rc, _, _, _ = cons_raw(reads, ks, [(0, 5, 3)], votes=votes)
        assert rc == _lib.ERR_ARG and "out of bounds" in lib.smx_last_error().decode()
        rc, _, _, _ = cons_raw(reads[:6], ks[:6], [(0, 0, 3), (0, 3, 3)], votes=votes)   # touching ranges, one draft
        assert rc == _lib.OK
    rc, _, _, _ = cons_raw(reads, ks, [(7, 0, 1)])
    assert rc == _lib.ERR_ARG and "out of bounds" in lib.smx_last_error().decode()
