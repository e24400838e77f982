"""The error-profile kernel on the GPU (smx_profile.hip through smx_cons_profile): the members' counts and the jobs' q /
subst / ins / hp tables of hand-made jobs against the plain-Python twin (errors_utils.profile_reference over
cons_utils.row_reference), compared with ==, at the edges of the 64-column batches, of the read-position carry, of the
run carry and its clamps, of the kept insertion codes, of the Phred bins and of the member slices of a workgroup.  Every
case also asserts on the twin's own rows that the situation it is named after is there."""
import random

import numpy as np
import pytest

from clusters_utils import rand_seq
from cons_utils import pair_limit, row_reference
from errors_utils import HP, INS, Q, SUBST, draft_runs, profile_reference
from specimux_amd import _lib, calls, consensus

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF
EDGE_QUALS = [32, 33, 96, 126, 34, 95, 97, 125]              # the bin edges 0 | 0, 63 | 63 and their neighbours


def profile_raw(reads, quals, ks, jobs, null=()):
    """One smx_cons_profile call with every output filled with a sentinel first; `null` names the arguments to pass as
    null.  -> (status, [(table, aligned, member words, tables)] per job, kernel ms, the raw outputs)."""
    roff, jarr = calls.offsets(reads), calls.job_array(jobs, _lib.CONS_JOB_DTYPE)
    words = [len(reads[d]) + 1 for d, _, _ in jobs]
    votes = np.full(max(sum(words) * 26, 1), SENTINEL, dtype=np.uint32)
    aligned = np.full(max(len(jobs), 1), SENTINEL, dtype=np.uint32)
    members = np.full(max(sum(n for _, _, n in jobs) * 8, 1), SENTINEL, dtype=np.uint32)
    tables = np.full(max(len(jobs) * 274, 1), SENTINEL, dtype=np.uint32)
    ms = []
    rc = calls.invoke("smx_cons_profile", b"".join(reads), _lib.ptr(roff), len(reads), _lib.ptr(np.array(ks, dtype=np.int32)),
                      _lib.ptr(jarr), len(jobs), None if "quals" in null else b"".join(quals), _lib.ptr(votes), _lib.ptr(aligned),
                      None if "per_member" in null else _lib.ptr(members), None if "tables" in null else _lib.ptr(tables),
                      kernel_ms=ms, check=False)
    raw = (votes, aligned, members, tables)
    if rc != _lib.OK:
        return rc, [], ms[0], raw
    out, at, mat = [], 0, 0
    for j, ((_d, _r0, n), w) in enumerate(zip(jobs, words)):
        out.append((votes[at * 26:(at + w) * 26].reshape(-1, 26), int(aligned[j]), members[mat * 8:(mat + n) * 8].reshape(n, 8),
                    tables[j * 274:(j + 1) * 274]))
        at, mat = at + w, mat + n
    return rc, out, ms[0], raw


def assert_equal(got, want):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g[1] == w[1] and np.array_equal(g[0], w[0]), j
        assert g[2].shape == w[2].shape and np.array_equal(g[2], w[2]), (j, np.argwhere(g[2] != w[2])[:5])
        assert np.array_equal(g[3], w[3]), (j, np.argwhere(g[3] != w[3])[:8], g[3][g[3] != w[3]][:8], w[3][g[3] != w[3]][:8])


def other_base(c, k=1):
    return "ACGT"[("ACGT".index(c) + k) % 4]


def plain(rng, m):
    """A draft of m bases without runs: no base equals its neighbour, so every indel below lands where it is made."""
    s = [rng.choice("ACGT")]
    while len(s) < m:
        s.append(rng.choice([c for c in "ACGT" if c != s[-1]]))
    return "".join(s)


class Call:
    def __init__(self):
        self.reads, self.quals, self.ks, self.jobs, self.names = [], [], [], [], {}

    def add(self, seq, k=20, qual=None):
        self.reads.append(seq.encode())
        self.quals.append(bytes(qual if qual is not None else [EDGE_QUALS[(i + len(self.reads)) % 8] for i in range(len(seq))]))
        self.ks.append(k)
        return len(self.reads) - 1

    def job(self, name, draft, members, draft_is_member=False):
        """members: [(sequence, k)]; the draft is member 0 of the job or a read of its own behind them."""
        r0 = len(self.reads)
        if draft_is_member:
            members = [(draft, 20)] + list(members)
        for s, k in members:
            self.add(s, k)
        d = r0 if draft_is_member else self.add(draft)
        self.names[name] = len(self.jobs)
        self.jobs.append((d, r0, len(members)))

    def row(self, name, i):
        d, r0, _n = self.jobs[self.names[name]]
        return row_reference(self.reads[d], self.reads[r0 + i], pair_limit(self.ks[d], self.ks[r0 + i]))


def sym(row, p):
    return row[p] & 7


def ins_len(row, p):
    return (row[p] >> 3) & 255


@pytest.fixture(scope="module")
def case():
    """One call with every job of this file, the twin's result and the GPU's."""
    rng = random.Random(211)
    c = Call()
    # -- drafts whose m + 1 words cross the batch edge both ways; the members carry an edit at every edge of the row
    for m in (63, 64, 65, 127, 128, 129):
        q = plain(rng, m)
        x = other_base(q[0], 2) if other_base(q[0], 2) != q[1] else other_base(q[0], 3)
        members = [(q, 20), (other_base(q[0]) + q[1:m - 1] + other_base(q[-1]), 20),            # subs at both ends
                   (x + q, 20), (q + other_base(q[-1]), 20), (q[1:], 20), (q[:-1], 20)]          # ins before 0, behind m - 1; dels
        for at in (63, 64):                                                                       # an insertion exactly at 63 / 64
            if at <= m:
                members.append((q[:at] + (other_base(q[at - 1]) if at == m or other_base(q[at - 1]) != q[at] else other_base(q[at - 1], 2))
                                + q[at:], 20))
        c.job("len%d" % m, q, members, draft_is_member=(m % 2 == 0))
    # -- runs: G x 5 over columns 62-66, A x 9 at 20-28 (class 8), members with the runs shorter and longer by up to 4 and 5
    q = list(plain(rng, 130))
    q[19], q[20:29], q[29] = "C", "A" * 9, "T"
    q[61], q[62:67], q[67] = "T", "G" * 5, "C"
    q = "".join(q)
    runs = [(q, 20)]
    for s, r in ((62, 5), (20, 9)):
        for d in (-4, -3, -1, 1, 3, 4, 5):
            runs.append((q[:s] + q[s] * (r + d) + q[s + r:], 20))
    c.job("runs", q, runs)
    # -- insertions of 3, 4 and 5 bases (kept codes against the overflow count), of a base that is not a neighbour's
    q = plain(rng, 100)
    lens = []
    for L, at in ((3, 10), (4, 50), (5, 64), (3, 0), (5, 100)):
        base = next(b for b in "ACGT" if b != q[max(at - 1, 0)] and b != q[min(at, 99)])
        lens.append((q[:at] + base * L + q[at:], 20))
    c.job("lens", q, lens, draft_is_member=True)
    # -- a 260-base insertion under no limit: clipped
    q = plain(rng, 130)
    base = next(b for b in "ACGT" if b != q[39] and b != q[40])
    c.job("clipped", q, [(q, 20), (q[:40] + base * 260 + q[40:], -1), (q[:100] + other_base(q[100]) + q[101:], 20)])
    # -- other bytes: N in the draft at 10 and 50, in a member at 30 and 50; an empty member; a member above its limit
    q = list(plain(rng, 90))
    q[10] = q[50] = "N"
    q = "".join(q)
    c.job("others", q, [(q, 20), (q[:10] + "A" + q[11:50] + "C" + q[51:], 20), (q[:30] + "N" + q[31:], 20), ("", -1),
                        (rand_seq(rng, 90), 5), (q[:10] + q[11:], 20)])
    # -- member counts around the waves' and workgroups' slices: 0, 1, 4, 5 and 65 members, noisy ones
    for n in (0, 1, 4, 5, 65):
        q = rand_seq(rng, 80)
        members = []
        for i in range(n - 1 if n in (4, 65) else n):          # those two have the draft as their member 0
            r = list(q)
            for _ in range(i % 7):
                p = rng.randrange(len(r))
                r[p:p + 1] = rng.choice(["", other_base(q[min(p, 79)]), r[p] + rng.choice("ACGT")])
            members.append(("".join(r) if i != 40 else rand_seq(rng, 80), 12))
        c.job("n%d" % n, q, members, draft_is_member=(n in (4, 65)))
    want = profile_reference(c.reads, c.quals, c.ks, c.jobs)
    rc, got, ms, _raw = profile_raw(c.reads, c.quals, c.ks, c.jobs)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert ms > 0
    return c, want, got


def job_of(case, name):
    c, want, got = case
    j = c.names[name]
    return c, want[j], got[j]


def test_the_whole_call_equals_the_twin(case):
    _c, want, got = case
    assert_equal(got, want)


@pytest.mark.parametrize("m", [63, 64, 65, 127, 128, 129])
def test_edits_at_the_edges_of_rows_and_batches(case, m):
    c, w, g = job_of(case, "len%d" % m)
    off = 1 if m % 2 == 0 else 0                               # the draft is member 0
    assert w[1] == len(w[2]) == (8 if m >= 64 else 7) + off
    words = w[2][off:]
    assert words[0].tolist() == [m, 0, 0, 0, 0, 0, 0, 0]
    assert words[1].tolist() == [m - 2, 2, 0, 0, 0, 0, 0, 0]
    assert ins_len(c.row("len%d" % m, off + 2)[1], 0) == 1 and words[2].tolist() == [m, 0, 0, 0, 1, 1, 0, 0]
    assert ins_len(c.row("len%d" % m, off + 3)[1], m) == 1 and words[3].tolist() == [m, 0, 0, 0, 1, 1, 0, 0]
    assert sym(c.row("len%d" % m, off + 4)[1], 0) == 5 and sym(c.row("len%d" % m, off + 5)[1], m - 1) == 5
    assert words[4].tolist() == words[5].tolist() == [m - 1, 0, 1, 0, 0, 0, 0, 0]
    for i, at in enumerate(a for a in (63, 64) if a <= m):
        assert ins_len(c.row("len%d" % m, off + 6 + i)[1], at) == 1, (m, at)
    assert np.array_equal(g[2], w[2]) and np.array_equal(g[3], w[3])
    # every read base is in q exactly once: the read positions met the reads' ends
    d, r0, n = c.jobs[c.names["len%d" % m]]
    assert int(w[3][Q:Q + 192].sum()) == sum(len(c.reads[r0 + i]) for i in range(n))
    assert {b for b in range(64) if w[3][Q + 3 * b:Q + 3 * b + 3].any()} == {0, 1, 62, 63}


def test_runs_across_a_batch_edge_class_8_and_the_clamps(case):
    c, w, g = job_of(case, "runs")
    d = c.jobs[c.names["runs"]][0]
    runs = draft_runs(c.reads[d])
    assert (62, 5, 2) in runs and (20, 9, 0) in runs and w[1] == 15
    hp = w[3][HP:].reshape(8, 7)
    # the run of 5: 7 members see it at -4 (clamped) .. +5 (clamped), the other 8 as it is; the run of 9 likewise in class 8
    assert hp[4].tolist() == [2, 0, 1, 8, 1, 0, 3] and hp[7].tolist() == [2, 0, 1, 8, 1, 0, 3]
    assert int(hp.sum()) == 15 * len(runs)
    assert np.array_equal(g[3], w[3]) and np.array_equal(g[2], w[2])


def test_kept_codes_and_the_overflow_count(case):
    c, w, g = job_of(case, "lens")
    assert [ins_len(c.row("lens", 1 + i)[1], at) for i, at in enumerate((10, 50, 64, 0, 100))] == [3, 4, 5, 3, 5]
    assert int(w[3][INS:INS + 5].sum()) == 3 + 4 + 4 + 3 + 4 and int(w[3][INS + 5]) == 2
    assert w[2][:, 4].tolist() == [0, 1, 1, 1, 1, 1] and w[2][:, 5].tolist() == [0, 3, 4, 5, 3, 5]
    assert int(w[3][Q:Q + 192].reshape(64, 3)[:, 2].sum()) == 20
    assert np.array_equal(g[3], w[3]) and np.array_equal(g[2], w[2])


def test_a_clipped_member_counts_everywhere_but_in_q(case):
    c, w, g = job_of(case, "clipped")
    assert ins_len(c.row("clipped", 1)[1], 40) == 255
    assert w[2].tolist() == [[130, 0, 0, 0, 0, 0, 0, 0], [130, 0, 0, 0, 1, 255, 1, 0], [129, 1, 0, 0, 0, 0, 0, 0]]
    assert int(w[3][SUBST:SUBST + 20].sum()) == 3 * 130 and int(w[3][INS:INS + 6].sum()) == 4 + 251
    assert int(w[3][Q:Q + 192].sum()) == 2 * 130               # two members' bases, none of the clipped member's 390
    assert int(w[3][HP:].sum()) == 3 * 130                     # the draft has no runs longer than 1: 130 runs per member
    assert np.array_equal(g[3], w[3]) and np.array_equal(g[2], w[2])


def test_other_bytes_an_empty_member_and_one_above_its_limit(case):
    c, w, g = job_of(case, "others")
    assert w[1] == 5
    assert w[2].tolist() == [[88, 0, 0, 2, 0, 0, 0, 0],       # N over N twice: other
                             [88, 0, 0, 2, 0, 0, 0, 0],       # a base over the draft's N: other
                             [87, 0, 0, 3, 0, 0, 0, 0],       # N over a base, and the two N over N
                             [0, 0, 90, 0, 0, 0, 0, 0],       # the empty member: all deletions
                             [0] * 8,                         # above its limit
                             [88, 0, 1, 1, 0, 0, 0, 0]]       # the deletion is at the draft's N: del, not other
    assert c.row("others", 4)[0] == -1 and sym(c.row("others", 5)[1], 10) == 5
    subst = w[3][SUBST:SUBST + 20].reshape(4, 5)
    assert int(subst.sum()) == 5 * 88 - 1 and int(subst[:, 4].sum()) == 88       # the N columns and the member's N are in no cell
    assert np.array_equal(g[3], w[3]) and np.array_equal(g[2], w[2])


@pytest.mark.parametrize("n", [0, 1, 4, 5, 65])
def test_member_counts_around_the_slices(case, n):
    c, w, g = job_of(case, "n%d" % n)
    assert g[2].shape == (n, 8) and w[1] == n - (1 if n == 65 else 0)
    if n == 65:
        assert not w[2][41].any()                              # the unrelated member, above its limit
    if n == 0:
        assert not w[3].any() and w[1] == 0
    assert np.array_equal(g[2], w[2]) and np.array_equal(g[3], w[3]) and np.array_equal(g[0], w[0]) and g[1] == w[1]


def test_votes_are_those_of_smx_cons_votes(case):
    c, _want, got = case
    tables, aligned = consensus.votes(c.reads, c.ks, c.jobs)
    assert aligned == [g[1] for g in got]
    for g, t in zip(got, tables):
        assert np.array_equal(g[0], t)


def test_the_same_call_twice_gives_identical_bytes(case):
    c, _want, _got = case
    a = profile_raw(c.reads, c.quals, c.ks, c.jobs)
    b = profile_raw(c.reads, c.quals, c.ks, c.jobs)
    assert a[0] == b[0] == _lib.OK
    for x, y in zip(a[3], b[3]):
        assert x.tobytes() == y.tobytes()
    assert not (a[3][2] == SENTINEL).any() and not (a[3][3] == SENTINEL).any()       # every word written


def test_null_arguments_are_refused_and_no_output_is_touched(case):
    c, _want, _got = case
    lib = _lib.load()
    for name in ("quals", "per_member", "tables"):
        rc, _out, _ms, raw = profile_raw(c.reads, c.quals, c.ks, c.jobs, null=(name,))
        assert rc == _lib.ERR_ARG and name in lib.smx_last_error().decode(), name
        assert all((x == SENTINEL).all() for x in raw)
    assert profile_raw(c.reads, c.quals, c.ks, [(0, 0, 10**6)])[0] == _lib.ERR_ARG
    # a call whose jobs have no members needs none of the three
    j = c.jobs[c.names["n0"]]
    rc, got, _ms, raw = profile_raw(c.reads, c.quals, c.ks, [j], null=("quals", "per_member"))
    assert rc == _lib.OK and got[0][1] == 0 and not got[0][3].any()
    rc, got, _ms, _raw = profile_raw(c.reads, c.quals, c.ks, [])
    assert rc == _lib.OK and got == []
