"""The resampling kernel on the GPU (smx_resample.hip through smx_cons_resample): the agree words and the replicates'
voters of hand-made jobs against the plain-Python twin (support_utils.resample_reference over cons_utils.row_reference),
compared with ==, at the edges of the member loop's unrolling, of the launch's column blocks, of the mask words and of
the tie rules.  The launch takes a workgroup row per (job, level) -- up to 2^31 - 1 of them, refused beyond -- and strides
over nothing, so no call here needs more jobs than a grid dimension holds."""
import random
import re

import numpy as np
import pytest

from clusters_utils import rand_seq
from cons_utils import votes_reference
from specimux_amd import _lib, calls, consensus
from support_utils import resample_reference

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF
SENTINEL64 = 0xDEADBEEFDEADBEEF
ONES = 2**64 - 1


def resample_raw(reads, ks, jobs, masks):
    """One smx_cons_resample call with every output filled with a sentinel first.  -> (status, [(table, aligned, agree,
    sub_aligned)] per job, kernel ms)."""
    roff, jarr = calls.offsets(reads), calls.job_array(jobs, _lib.CONS_JOB_DTYPE)
    masks = np.ascontiguousarray(masks, dtype=np.uint64)
    n_levels = masks.shape[0]
    words = [len(reads[d]) + 1 for d, _, _ in jobs]
    votes = np.full(max(sum(words) * 26, 1), SENTINEL, dtype=np.uint32)
    aligned = np.full(max(len(jobs), 1), SENTINEL, dtype=np.uint32)
    agree = np.full(max(sum(words) * n_levels, 1), SENTINEL64, dtype=np.uint64)
    sub = np.full(max(len(jobs) * n_levels * 64, 1), SENTINEL, dtype=np.uint32)
    ms = []
    rc = calls.invoke("smx_cons_resample", b"".join(reads), _lib.ptr(roff), len(reads), _lib.ptr(np.array(ks, dtype=np.int32)),
                      _lib.ptr(jarr), len(jobs), _lib.ptr(masks) if masks.size else None, n_levels, _lib.ptr(votes),
                      _lib.ptr(aligned), _lib.ptr(agree), _lib.ptr(sub), kernel_ms=ms, check=False)
    if rc != _lib.OK:
        return rc, [], ms[0]
    out, at = [], 0
    for j, w in enumerate(words):
        out.append((votes[at * 26:(at + w) * 26].reshape(-1, 26), int(aligned[j]),
                    agree[at * n_levels:(at + w) * n_levels].reshape(n_levels, w),
                    sub[j * n_levels * 64:(j + 1) * n_levels * 64].reshape(n_levels, 64)))
        at += w
    assert at * n_levels == agree.size or not jobs
    return rc, out, ms[0]


def assert_equal(got, want):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g[1] == w.aligned and np.array_equal(g[0], w.table), j
        assert g[2].shape == w.agree.shape and np.array_equal(g[2], w.agree), (j, np.argwhere(g[2] != w.agree)[:5])
        assert np.array_equal(g[3], w.sub_aligned), (j, np.argwhere(g[3] != w.sub_aligned)[:5])


def with_bases(seq, edits):
    s = list(seq)
    for p, c in edits.items():
        s[p] = c
    return "".join(s)


def other_base(c, k=1):
    return "ACGT"[("ACGT".index(c) + k) % 4]


def level_masks(rng, total, n_levels):
    """The mask words of a call: level 0 all zero, 1 all ones, 2 bit 0 alone, 3 bit 63 alone, the rest random of falling
    density; fewer levels take the last of these."""
    shapes = [lambda: 0, lambda: ONES, lambda: 1, lambda: 1 << 63, lambda: rng.getrandbits(64),
              lambda: rng.getrandbits(64) | rng.getrandbits(64), lambda: rng.getrandbits(64) & rng.getrandbits(64)]
    rows = []
    for l in range(16):
        f = shapes[l] if l < len(shapes) else shapes[4 + l % 3]
        rows.append([f() for _ in range(total)])
    return np.array(rows[16 - n_levels:], dtype=np.uint64).reshape(n_levels, total)


@pytest.fixture(scope="module")
def sizes():
    """One call of 16 levels: jobs of 1, 63, 64, 65 and 129 members around 70-nt drafts -- a third of the members carry a
    second allele at two positions, one member in five has an error of its own -- and a job without members between them.
    Member 30 of the job of 65 is an unrelated read above its limit, and the masks include it.  With the twin's result."""
    rng = random.Random(181)
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
    masks = level_masks(rng, sum(n for _, _, n in jobs), 16)
    return raw, ks, jobs, masks, resample_reference(raw, ks, jobs, masks)


def test_member_counts_mask_shapes_and_an_unaligned_member(sizes):
    reads, ks, jobs, masks, want = sizes
    rc, got, ms = resample_raw(reads, ks, jobs, masks)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert ms > 0
    assert_equal(got, want)
    # what the twin must have seen for the comparison to cover the edges
    assert [w.aligned for w in want] == [1, 63, 64, 0, 64, 129]
    for j, w in enumerate(want):
        n = jobs[j][2]
        assert w.sub_aligned[0].tolist() == [0] * 64 and w.agree[0].tolist() == [ONES] * 71      # no voters: every column kept
        # all ones: the 64 replicates are the same, and the draft is what its members call
        assert w.sub_aligned[1].tolist() == [w.aligned] * 64 and w.agree[1].tolist() == [ONES] * 71
        assert w.sub_aligned[2].tolist() == [w.aligned] + [0] * 63 and w.sub_aligned[3].tolist() == [0] * 63 + [w.aligned]
        assert {int(x) for x in w.agree[2]} == {ONES} == {int(x) for x in w.agree[3]}
        if n == 0:
            assert (w.agree == np.uint64(ONES)).all() and not w.sub_aligned.any()
    # the unrelated member of the job of 65 is in every replicate of level 1 and votes in none: 64 voters of 65 members
    assert want[4].sub_aligned[1, 0] == 64 < jobs[4][2]
    at = sum(n for _, _, n in jobs[:4]) + 30
    for l in range(4, 16):
        holds = [(int(masks[l, at]) >> b) & 1 for b in range(64)]
        size = [sum((int(w) >> b) & 1 for w in masks[l, at - 30:at + 35]) for b in range(64)]
        assert [int(x) for x in want[4].sub_aligned[l]] == [s - h for s, h in zip(size, holds)] and sum(holds) > 5
    # the random levels clear bits at the two sites of the larger jobs, and only in some replicates
    for j in (1, 2, 4, 5):
        cleared = [p for p in range(71) if any(int(want[j].agree[l, p]) != ONES for l in range(4, 16))]
        assert {20, 50} <= set(cleared), (j, cleared)
    # no atomics: the same from run to run
    again = resample_raw(reads, ks, jobs, masks)
    for g, a in zip(got, again[1]):
        assert all(np.array_equal(x, y) for x, y in zip(g[2:], a[2:])) and np.array_equal(g[0], a[0])


def test_votes_are_those_of_smx_cons_votes_and_one_level(sizes):
    reads, ks, jobs, masks, want = sizes
    one = masks[15:16]
    rc, got, _ms = resample_raw(reads, ks, jobs, one)
    assert rc == _lib.OK
    tables, aligned = consensus.votes(reads, ks, jobs)
    assert aligned == [g[1] for g in got]
    for g, t, w in zip(got, tables, want):
        assert np.array_equal(g[0], t)
        assert g[2].shape == (1, 71) and np.array_equal(g[2][0], w.agree[15]) and np.array_equal(g[3][0], w.sub_aligned[15])


def test_one_workgroup_path(sizes, monkeypatch):
    """A history workspace of one slice, as in the cons tests: the alignment runs as one workgroup over all chunks."""
    reads, ks, jobs, masks, want = sizes
    monkeypatch.setenv("SMX_CONS_HIST_BYTES", "1")
    rc, _, _ = resample_raw(reads, ks, jobs, masks)
    msg = _lib.load().smx_last_error().decode()
    assert rc == _lib.ERR_UNSUPPORTED and "history" in msg, (rc, msg)
    monkeypatch.setenv("SMX_CONS_HIST_BYTES", re.search(r"needs (\d+) bytes", msg).group(1))
    rc, got, _ms = resample_raw(reads, ks, jobs, masks)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert_equal(got, want)


def test_draft_lengths_around_the_column_blocks():
    """Drafts of 1, 255, 256 and 257 bases, ten members each (and so two rounds and a half of the member loop): four are
    the draft, three carry another base at p = 0 and p = m - 1, three an extra base behind the last one.  Random masks:
    some replicates drop p = 0 and p = m - 1, some emit the insertion at p = m."""
    rng = random.Random(182)
    reads, ks, jobs = [], [], []
    for m in (1, 255, 256, 257):
        q = rand_seq(rng, m)
        b = with_bases(q, {0: other_base(q[0]), m - 1: other_base(q[m - 1])})
        c = q + other_base(q[m - 1], 2)
        jobs.append((len(reads) + 10, len(reads), 10))
        reads += [q] * 4 + [b] * 3 + [c] * 3 + [q]
        ks += [-1] * 11
    raw = [r.encode() for r in reads]
    masks = np.array([[rng.getrandbits(64) & rng.getrandbits(64) for _ in range(40)] for _ in range(2)], dtype=np.uint64)
    want = resample_reference(raw, ks, jobs, masks)
    for (d, _r0, _n), w in zip(jobs, want):
        m = len(raw[d])
        cleared = {p for p in range(m + 1) if any(int(w.agree[l, p]) != ONES for l in range(2))}
        assert cleared == {0, m - 1, m}, (m, cleared)
        assert all(0 < bin(int(w.agree[l, p])).count("1") < 64 for l in range(2) for p in cleared)
    rc, got, _ms = resample_raw(raw, ks, jobs, masks)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert_equal(got, want)


def test_ties_and_other_bytes():
    """20 members of a 60-nt draft with `N` at p = 40 and p = 45, under all-ones masks (every replicate is the full vote)
    and random ones.  p = 10: ten A and ten C, the draft has A -- the draft wins a tie it is part of.  p = 25: ten A and ten
    C, the draft has G -- a tie without the draft.  p = 30: ten members lack the base -- exactly half deletions keep it.
    p = 40: all members have N -- no vote for a base, the draft's byte stands.  p = 45: the members have A.  p = 50: ten
    members have an extra base before it -- exactly half insertions emit nothing."""
    rng = random.Random(183)
    q = rand_seq(rng, 60)
    q = with_bases(q, {10: "A", 25: "G", 29: "A", 30: "C", 31: "G", 40: "N", 45: "N", 49: "A", 50: "C"})
    reads = []
    for i in range(20):
        r = with_bases(q, {10: "A" if i < 10 else "C", 25: "A" if i % 2 else "C", 45: "A"})
        r = r[:50] + ("T" if i % 2 else "") + r[50:]
        r = r[:30] + ("" if i % 4 < 2 else "C") + r[31:]
        reads.append(r.encode())
    reads.append(q.encode())
    ks, jobs = [10] * 21, [(20, 0, 20)]
    table = votes_reference(reads, ks, jobs)[0][0]
    assert table[10, :4].tolist() == [10, 10, 0, 0] and table[25, :4].tolist() == [10, 10, 0, 0]
    assert table[30, 5] == 10 and table[30, 1] == 10 and table[40, 4] == 20 and table[45, 0] == 20 and table[50, 6:11].sum() == 10
    masks = np.array([[ONES] * 20, [rng.getrandbits(64) for _ in range(20)], [rng.getrandbits(64) for _ in range(20)]],
                     dtype=np.uint64)
    want = resample_reference(reads, ks, jobs, masks)
    full = [int(w) for w in want[0].agree[0]]
    assert [p for p in range(61) if full[p] != ONES] == [25, 45] and full[25] == full[45] == 0
    for p in (10, 30, 50):                                     # the ties fall either way in the random subsets
        assert all(0 < bin(int(want[0].agree[l, p])).count("1") < 64 for l in (1, 2)), p
    assert int(want[0].agree[1, 40]) == ONES and int(want[0].agree[1, 45]) == 0
    rc, got, _ms = resample_raw(reads, ks, jobs, masks)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert_equal(got, want)


def test_bad_arguments_are_rejected(sizes):
    reads, ks, jobs, masks, _want = sizes
    lib = _lib.load()
    total = masks.shape[1]
    for n_levels in (0, 17):
        assert resample_raw(reads, ks, jobs, np.zeros((n_levels, total), dtype=np.uint64))[0] == _lib.ERR_ARG
        assert "n_levels" in lib.smx_last_error().decode()
    assert resample_raw(reads, ks, [], np.zeros((17, 0), dtype=np.uint64))[0] == _lib.ERR_ARG
    assert resample_raw(reads, ks, [(0, 0, 400)], masks)[0] == _lib.ERR_ARG and "out of bounds" in lib.smx_last_error().decode()
    rc, got, _ms = resample_raw(reads, ks, [], masks[:, :0])
    assert rc == _lib.OK and got == []
    # a call whose jobs have no members needs no masks
    rc, got, _ms = resample_raw(reads, ks, [jobs[3]], np.zeros((2, 0), dtype=np.uint64))
    assert rc == _lib.OK and (got[0][2] == np.uint64(ONES)).all() and not got[0][3].any() and got[0][1] == 0
