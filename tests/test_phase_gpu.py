"""The variant kernels on the GPU (smx_phase.hip through smx_cons_phase): sites, allele planes and link tables of hand-made
jobs against the plain-Python twin (variants_utils.phase_reference over cons_utils.row_reference), every table compared
with ==, at the edges of the plane words, of the site walk, of the thresholds and of the tie rules."""
import random
import re

import numpy as np
import pytest

from clusters_utils import rand_seq
from specimux_amd import _lib, calls, consensus
from specimux_amd.variants import JobPhase, Site
from variants_utils import phase_reference

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF


def phase_raw(reads, ks, jobs, min_permille, min_reads, max_sites):
    """One smx_cons_phase call with every output filled with a sentinel first.  -> (status, [JobPhase], site slots past
    the kept ones, kernel ms)."""
    roff, jarr = calls.offsets(reads), calls.job_array(jobs, _lib.CONS_JOB_DTYPE)
    vwords = [(len(reads[d]) + 1) * 26 for d, _, _ in jobs]
    pwords = [(n + 63) // 64 for _, _, n in jobs]
    votes = np.full(max(sum(vwords), 1), SENTINEL, dtype=np.uint32)
    aligned = np.full(max(len(jobs), 1), SENTINEL, dtype=np.uint32)
    sites = np.frombuffer(np.full(max(len(jobs) * max_sites, 1) * 4, SENTINEL, dtype=np.uint32).tobytes(),
                          dtype=_lib.CONS_SITE_DTYPE).copy()
    n_sites = np.full(max(len(jobs), 1), SENTINEL, dtype=np.uint32)
    n_qualified = np.full(max(len(jobs), 1), SENTINEL, dtype=np.uint32)
    planes = np.full(max(sum(pwords) * 2 * max_sites, 1), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    link = np.full(max(len(jobs) * max_sites * max_sites * 4, 1), SENTINEL, dtype=np.uint32)
    ms = []
    rc = calls.invoke("smx_cons_phase", b"".join(reads), _lib.ptr(roff), len(reads), _lib.ptr(np.array(ks, dtype=np.int32)),
                      _lib.ptr(jarr), len(jobs), min_permille, min_reads, max_sites, _lib.ptr(votes), _lib.ptr(aligned),
                      _lib.ptr(sites), _lib.ptr(n_sites), _lib.ptr(n_qualified), _lib.ptr(planes), _lib.ptr(link), kernel_ms=ms,
                      check=False)
    if rc != _lib.OK:
        return rc, [], None, ms[0]
    out, spare, vat, pat = [], [], 0, 0
    for j, (vw, pw) in enumerate(zip(vwords, pwords)):
        slots = sites[j * max_sites:(j + 1) * max_sites]
        kept = [Site(*(int(s[f]) for f in ("pos", "kind", "major", "minor", "n_major", "n_minor"))) for s in slots[:n_sites[j]]]
        spare.append(slots[n_sites[j]:])
        out.append(JobPhase(votes[vat:vat + vw].reshape(-1, 26), int(aligned[j]), kept, int(n_qualified[j]),
                            planes[pat:pat + max_sites * 2 * pw].reshape(max_sites, 2, pw),
                            link[j * max_sites ** 2 * 4:(j + 1) * max_sites ** 2 * 4].reshape(max_sites, max_sites, 4)))
        vat, pat = vat + vw, pat + max_sites * 2 * pw
    assert vat == votes.size or not jobs
    return rc, out, spare, ms[0]


def assert_equal(got, spare, want):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.aligned == w.aligned and np.array_equal(g.table, w.table), j
        assert g.sites == w.sites and g.n_qualified == w.n_qualified, (j, g.sites, w.sites, g.n_qualified, w.n_qualified)
        assert g.planes.shape == w.planes.shape and np.array_equal(g.planes, w.planes), (j, np.argwhere(g.planes != w.planes)[:5])
        assert np.array_equal(g.link, w.link), (j, np.argwhere(g.link != w.link)[:5])
        assert not np.frombuffer(spare[j].tobytes(), dtype=np.uint8).any(), j      # the slots past the kept sites are zero


def with_bases(seq, edits):
    s = list(seq)
    for p, c in edits.items():
        s[p] = c
    return "".join(s)


def other_base(c, k=1):
    return "ACGT"[("ACGT".index(c) + k) % 4]


@pytest.fixture(scope="module")
def sizes():
    """One call: jobs of 1, 63, 64, 65 and 129 members around 70-nt drafts -- a third of the members carry a second allele
    at two positions, one member in five has an error of its own -- and a job without members between them.  Member 30 of
    the job of 65, in the middle of its first word, is an unrelated read above its limit.  With the twin's result."""
    rng = random.Random(81)
    reads, ks, jobs = [], [], []
    for n in (1, 63, 64, 0, 65, 129):
        q = rand_seq(rng, 70)
        b = with_bases(q, {20: other_base(q[20]), 50: other_base(q[50])})
        jobs.append((len(reads), len(reads), n))
        for i in range(n):
            r = b if i % 3 == 1 else q
            if i % 5 == 4:
                p = rng.randrange(70)
                r = with_bases(r, {p: other_base(r[p], 2)})
            if n == 65 and i == 30:
                r = rand_seq(rng, 70)
            reads.append(r)
        ks += [10] * n
    reads.append(rand_seq(rng, 70))                            # the draft of the job without members
    ks.append(10)
    jobs[3] = (len(reads) - 1, jobs[3][1], 0)
    raw = [r.encode() for r in reads]
    return raw, ks, jobs, phase_reference(raw, ks, jobs, 150, 2, 8)


def test_member_counts_and_an_unaligned_member(sizes):
    reads, ks, jobs, want = sizes
    rc, got, spare, ms = phase_raw(reads, ks, jobs, 150, 2, 8)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert ms > 0
    assert_equal(got, spare, want)
    # what the twin must have seen for the comparison to cover the edges
    assert [w.aligned for w in want] == [1, 63, 64, 0, 64, 129]
    assert want[0].sites == [] and want[3].sites == [] and want[3].n_qualified == 0 and want[3].planes.shape == (8, 2, 0)
    for j in (1, 2, 4, 5):
        assert [(s.pos, s.kind) for s in want[j].sites] == [(20, 0), (50, 0)], j
        n11, n10, n01, n00 = (int(x) for x in want[j].link[0, 1])
        assert n10 == n01 == 0 and n11 >= 20 and n00 >= 40
    assert [w.planes.shape[2] for w in want] == [1, 1, 1, 0, 2, 3]
    both = want[4].planes[:, 0, 0] | want[4].planes[:, 1, 0]
    assert not ((both >> np.uint64(30)) & np.uint64(1)).any() and ((both[:2] >> np.uint64(31)) & np.uint64(1)).all()
    assert int(want[4].planes[1, 0, 1]) | int(want[4].planes[1, 1, 1]) == 1    # member 64: bit 0 of the second word
    assert int(want[5].planes[0, 0, 2]) | int(want[5].planes[0, 1, 2]) == 1    # member 128: the third word
    # no atomics: the same from run to run
    again = phase_raw(reads, ks, jobs, 150, 2, 8)
    assert_equal(again[1], again[2], got)


def test_votes_are_those_of_smx_cons_votes(sizes):
    reads, ks, jobs, want = sizes
    rc, got, _spare, _ms = phase_raw(reads, ks, jobs, 150, 2, 8)
    assert rc == _lib.OK
    tables, aligned = consensus.votes(reads, ks, jobs)
    assert aligned == [g.aligned for g in got]
    for g, t in zip(got, tables):
        assert np.array_equal(g.table, t)


def test_one_workgroup_path(sizes, monkeypatch):
    """A history workspace of one slice, as in the cons tests: the alignment runs as one workgroup over all chunks."""
    reads, ks, jobs, want = sizes
    monkeypatch.setenv("SMX_CONS_HIST_BYTES", "1")
    rc, _, _, _ = phase_raw(reads, ks, jobs, 150, 2, 8)
    msg = _lib.load().smx_last_error().decode()
    assert rc == _lib.ERR_UNSUPPORTED and "history" in msg, (rc, msg)
    monkeypatch.setenv("SMX_CONS_HIST_BYTES", re.search(r"needs (\d+) bytes", msg).group(1))
    rc, got, spare, _ms = phase_raw(reads, ks, jobs, 150, 2, 8)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert_equal(got, spare, want)


def test_site_positions():
    """A 300-nt draft, 20 members: six carry substitutions at p = 0, 255, 256 (the second round of the site walk) and
    299 = m - 1, four others an extra base behind the last one: the insertion site at p = m."""
    rng = random.Random(82)
    q = rand_seq(rng, 300)
    b = with_bases(q, {p: other_base(q[p]) for p in (0, 255, 256, 299)})
    c = q + other_base(q[299])
    reads = [r.encode() for r in [q] * 10 + [b] * 6 + [c] * 4]
    ks, jobs = [30] * 20, [(0, 0, 20)]
    want = phase_reference(reads, ks, jobs, 150, 2, 16)
    assert [(s.pos, s.kind, s.n_major, s.n_minor) for s in want[0].sites] == \
        [(0, 0, 14, 6), (255, 0, 14, 6), (256, 0, 14, 6), (299, 0, 14, 6), (300, 1, 16, 4)]
    assert want[0].link[0, 3].tolist() == [6, 0, 0, 14] and want[0].link[3, 4].tolist() == [0, 6, 4, 10]
    rc, got, spare, _ms = phase_raw(reads, ks, jobs, 150, 2, 16)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert_equal(got, spare, want)


@pytest.fixture(scope="module")
def counted():
    """A 60-nt draft and 20 members of its length: 2 members differ at p = 10, 3 others at p = 20, 4 others at p = 30."""
    rng = random.Random(83)
    q = rand_seq(rng, 60)
    reads = [q] * 20
    for members, p in ((range(0, 2), 10), (range(2, 5), 20), (range(5, 9), 30)):
        for i in members:
            reads[i] = with_bases(q, {p: other_base(q[p])})
    return [r.encode() for r in reads + [q]], [6] * 21, [(20, 0, 20)]


@pytest.mark.parametrize("min_permille,min_reads,max_sites,kept,qualified", [
    (150, 2, 8, [20, 30], 2),      # 3 of 20 is 150 per mille exactly; 2 of 20 is one vote under it
    (200, 2, 8, [30], 1),          # 4 of 20 is 200 per mille exactly; 3 of 20 is one vote under it
    (150, 3, 8, [20, 30], 2),      # 3 reads on min_reads = 3
    (150, 4, 8, [30], 1),          # 4 reads on min_reads = 4; 3 reads one under it, with share enough
    (100, 2, 8, [10, 20, 30], 3),
    (100, 2, 2, [10, 20], 3),      # three qualify, max_sites = 2: the first two are kept
    (100, 2, 1, [10], 3),
    (1000, 0, 8, [], 0),
])
def test_thresholds_and_clipping(counted, min_permille, min_reads, max_sites, kept, qualified):
    reads, ks, jobs = counted
    want = phase_reference(reads, ks, jobs, min_permille, min_reads, max_sites)
    assert [s.pos for s in want[0].sites] == kept and want[0].n_qualified == qualified
    rc, got, spare, _ms = phase_raw(reads, ks, jobs, min_permille, min_reads, max_sites)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert_equal(got, spare, want)


def test_ties_and_other_bytes():
    """20 members of a 60-nt draft.  p = 10: ten A and ten C, a tie for major -- the lower code is major.  p = 25: ten A,
    five G, five T, a tie for minor -- the lower code is minor.  p = 40: twelve A, five C and three N -- `other` is no
    allele and its members have neither bit.  p = 50: ten reads with an insertion before it and ten without, a tie --
    `present` is minor."""
    rng = random.Random(84)
    q = with_bases(rand_seq(rng, 60), {10: "A", 25: "A", 40: "A"})
    reads = []
    for i in range(20):
        r = with_bases(q, {10: "A" if i < 10 else "C", 25: "A" if i % 2 else ("G" if i % 4 else "T"),
                           40: "N" if i in (3, 4, 17) else ("C" if i in (5, 6, 7, 8, 9) else "A")})
        if i % 2:
            r = r[:50] + other_base(q[49], 2 if other_base(q[49], 2) != q[50] else 1) + r[50:]
        reads.append(r.encode())
    reads.append(q.encode())
    ks, jobs = [10] * 21, [(20, 0, 20)]
    want = phase_reference(reads, ks, jobs, 150, 2, 8)
    assert want[0].sites == [Site(10, 0, 0, 1, 10, 10), Site(25, 0, 0, 2, 10, 5), Site(40, 0, 0, 1, 12, 5),
                             Site(50, 1, 0, 1, 10, 10)]
    n_bits = int(want[0].planes[2, 0, 0]) | int(want[0].planes[2, 1, 0])
    assert [i for i in range(20) if not (n_bits >> i) & 1] == [3, 4, 17]
    rc, got, spare, _ms = phase_raw(reads, ks, jobs, 150, 2, 8)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert_equal(got, spare, want)


def test_many_sites_fill_the_largest_table():
    """max_sites = 64 with more than 64 qualifying candidates, spread over both rounds of a 300-nt draft's site walk and
    all four waves of a round: the compaction keeps the order and stops at 64."""
    rng = random.Random(85)
    q = rand_seq(rng, 300)
    at = list(range(2, 300, 4))                                # 75 positions
    b = with_bases(q, {p: other_base(q[p]) for p in at})
    reads = [r.encode() for r in [q] * 6 + [b] * 4]
    ks, jobs = [-1] * 10, [(0, 0, 10)]
    want = phase_reference(reads, ks, jobs, 300, 2, 64)
    assert [s.pos for s in want[0].sites] == at[:64] and want[0].n_qualified == 75
    rc, got, spare, _ms = phase_raw(reads, ks, jobs, 300, 2, 64)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert_equal(got, spare, want)


def test_bad_arguments_are_rejected(counted):
    reads, ks, jobs = counted
    lib = _lib.load()
    for max_sites in (0, 65):
        assert phase_raw(reads, ks, jobs, 150, 2, max_sites)[0] == _lib.ERR_ARG and "max_sites" in lib.smx_last_error().decode()
    assert phase_raw(reads, ks, jobs, 1001, 2, 8)[0] == _lib.ERR_ARG and "min_permille" in lib.smx_last_error().decode()
    assert phase_raw(reads, ks, [(0, 0, 30)], 150, 2, 8)[0] == _lib.ERR_ARG and "out of bounds" in lib.smx_last_error().decode()
    rc, got, _spare, _ms = phase_raw(reads, ks, [], 150, 2, 8)
    assert rc == _lib.OK and got == []
