"""The crosstalk kernel on the GPU (smx_nearest.hip): smx_nearest_distances against the suite's oracle over refs of every
state class, the generic one and a ref of 4 097 bases, jobs of 1 / 127 / 128 / 129 / 257 reads, limits at d - 1, d, d + 1,
empty reads and identical refs; smx_nearest's two arrays == a host reduction of those distances with one run per class and
with runs of one ref; two calls give the same arrays; bad arguments are refused with a message."""
import random

import numpy as np
import pytest

from oracle.edlib_semantics import NW, align_c
from specimux_amd import _lib, calls, crosstalk

pytestmark = pytest.mark.gpu

SHORT, LONG = (1, 63, 64, 65, 128, 129), (1024, 1025, 1100, 4097)


def mutate(rng, s, rate, alpha):
    out = []
    for c in s:
        r = rng.random()
        if r < rate / 3:
            out.append(rng.choice(alpha))
        elif r < 2 * rate / 3:
            out.append(c + rng.choice(alpha))
        elif r >= rate:
            out.append(c)
    return "".join(out)


def build_case(alpha, seed):
    """Thirteen refs -- the short ones, a twin of the 64-base ref in its group and a twin of the 65-base ref in another,
    the long ones, a twin of the 1 024-base ref in its group -- and jobs of 1 and 127 reads over all refs (two reads
    per long ref, so that the oracle stays quick), 128 and 129 reads over the eight short refs, 257 over six of them."""
    rng = random.Random(seed)
    refs = ["".join(rng.choice(alpha) for _ in range(m)) for m in SHORT]
    groups = list(range(len(refs)))
    refs += [refs[2], refs[3]]
    groups += [2, 100]
    n_short = len(refs)
    for m in LONG:
        refs.append("".join(rng.choice(alpha) for _ in range(m)))
        groups.append(len(refs) - 1)
    refs.append(refs[n_short])
    groups.append(groups[n_short])
    nq = len(refs)
    seqs, ks, edge, jobs = list(refs), [len(r) // 10 for r in refs], [None] * nq, []
    for nt, (q0, n) in ((1, (0, nq)), (127, (0, nq)), (128, (0, n_short)), (129, (0, n_short)), (257, (1, 6))):
        t0 = len(seqs)
        for i in range(nt):
            src = n_short + i // 2 if (q0, n) == (0, nq) and nt > 1 and i < 2 * len(LONG) else q0 + rng.randrange(min(n, n_short))
            kind = rng.randrange(12)
            e = None
            if kind == 0:
                s, k = "", rng.choice((-1, len(refs[src])))
            elif kind == 1:
                s = "".join(rng.choice(alpha) for _ in range(len(refs[src]) + rng.randrange(4)))
                k = len(s) // 10
            elif kind == 2:
                s, k = refs[src], 0
            elif kind <= 5:
                s, k, e = mutate(rng, refs[src], 0.05, alpha), 0, kind - 4
            elif kind == 6:
                s, k = mutate(rng, refs[src], 0.05, alpha), -1
            else:
                s = mutate(rng, refs[src], 0.01 * rng.randrange(12), alpha)
                k = len(s) // 10
            seqs.append(s)
            ks.append(k)
            edge.append(e)
            groups.append(groups[src] if rng.randrange(4) else rng.choice(groups[:nq] + [7777]))
        jobs.append((q0, n, t0, nt))
    jobs.append((0, nq, 0, 0))                     # no reads
    seqs += [refs[0], ""]                          # and a job without refs: its two reads keep both keys all-ones
    ks += [-1, 3]
    groups += [0, 0]
    edge += [None, None]
    jobs.append((0, 0, len(seqs) - 2, 2))
    return refs, seqs, ks, groups, edge, jobs


def oracle_distances(seqs, jobs):
    out = []
    for q0, nq, t0, nt in jobs:
        d = np.zeros((nq, nt), dtype=np.int64)
        for q in range(nq):
            for t in range(nt):
                a, b = seqs[q0 + q], seqs[t0 + t]
                d[q, t] = align_c(a, b, NW, -1, iupac=False)["editDistance"] if b else len(a)
        out.append(d)
    return out


@pytest.fixture(scope="module", params=["ACGT", "ACGTNRY"])
def case(request):
    """The case, the oracle's unlimited distances (computed once) and the limited distances expected of the device."""
    refs, seqs, ks, groups, edge, jobs = build_case(request.param, 5 + len(request.param))
    full = oracle_distances(seqs, jobs)
    for (q0, nq, t0, nt), d in zip(jobs, full):    # limits at the nearest ref's distance - 1, + 0, + 1 (over refs with k <= that)
        for t in range(nt):
            if edge[t0 + t] is not None and nq:
                ks[t0 + t] = max(0, int(d[:, t].min()) + edge[t0 + t])
    want, hits = [], {-1: 0, 0: 0, 1: 0}
    for (q0, nq, t0, nt), d in zip(jobs, full):
        w = np.empty((nq, nt), dtype=np.int32)
        for q in range(nq):
            for t in range(nt):
                k = -1 if ks[q0 + q] < 0 or ks[t0 + t] < 0 else max(ks[q0 + q], ks[t0 + t])
                w[q, t] = d[q, t] if k < 0 or d[q, t] <= k else -1
                if k - int(d[q, t]) in hits:
                    hits[k - int(d[q, t])] += 1
        want.append(w)
    assert min(hits.values()) >= 20, hits          # the limit at d - 1, d, d + 1 of some pair
    b = [s.encode("latin-1") for s in seqs]
    return b, ks, groups, jobs, want


def test_distances_match_the_oracle(case):
    seqs, ks, groups, jobs, want = case
    got = crosstalk.nearest_distances(seqs, ks, groups, jobs)      # prefilled with a sentinel (-7)
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and not (g == -7).any(), j
        bad = np.argwhere(g != w)
        assert bad.size == 0, (j, jobs[j], bad[:5].tolist(), [(int(g[q, t]), int(w[q, t])) for q, t in bad[:5]])
    assert sum(int((w >= 0).sum()) for w in want) >= 600 and sum(int((w < 0).sum()) for w in want) >= 2000


def test_distances_walk_over_many_short_runs(monkeypatch):
    """The chunk walk (smx_mine_lds.h) where it can go wrong, all in state class 1: 701 jobs over six shared refs with runs
    of one ref, more than 4096 runs, so that the owner search takes its third round; runs of two, three and one chunk
    (jobs of 129, 257 and 1 reads), one chunk per workgroup, so that most workgroups start inside a run.  The reads are
    drawn from a small pool, so the oracle aligns every distinct pair once; every distance of the call is compared."""
    monkeypatch.setenv("SMX_NEAREST_MIN_CHUNKS", "18446744073709551615")      # runs of one ref
    rng = random.Random(9)
    refs = ["".join(rng.choice("ACGT") for _ in range(rng.randrange(12, 41))) for _ in range(6)]
    pool = [(mutate(rng, rng.choice(refs), 0.02 * rng.randrange(10), "ACGT") or "A")[:40].ljust(12, "A") for _ in range(40)]
    kref, kpool = [rng.choice((-1, 2, 5)) for _ in refs], [rng.choice((-1, 1, 4, 8)) for _ in pool]
    table = np.empty((len(refs), len(pool)), dtype=np.int32)
    for q, a in enumerate(refs):
        for t, b in enumerate(pool):
            d = align_c(a, b, NW, -1, iupac=False)["editDistance"]
            k = -1 if kref[q] < 0 or kpool[t] < 0 else max(kref[q], kpool[t])
            table[q, t] = d if k < 0 or d <= k else -1
    sizes = [(129, 257, 1, 257)[j % 4] for j in range(701)]
    ids = np.array([rng.randrange(len(pool)) for _ in range(sum(sizes))])
    jobs, t0 = [], len(refs)
    for nt in sizes:
        jobs.append((0, len(refs), t0, nt))
        t0 += nt
    per_run = [(nt + 127) // 128 for nt in sizes for _ in refs]               # the chunks of every run, in launch order
    assert len(per_run) > 4096 and sum(per_run) - len(per_run) > sum(per_run) // 2
    seqs = [s.encode("latin-1") for s in refs + [pool[x] for x in ids]]
    ks = kref + [kpool[x] for x in ids]
    got = crosstalk.nearest_distances(seqs, ks, [0] * len(seqs), jobs)         # prefilled with a sentinel (-7)
    assert len(got) == len(jobs)
    n_in = n_out = 0
    for j, (g, (_, _, t0, nt)) in enumerate(zip(got, jobs)):
        w = table[:, ids[t0 - len(refs):t0 - len(refs) + nt]]
        bad = np.argwhere(g != w)
        assert g.shape == w.shape and bad.size == 0, (j, jobs[j], bad[:5].tolist(), [(int(g[q, t]), int(w[q, t])) for q, t in bad[:5]])
        n_in, n_out = n_in + int((w >= 0).sum()), n_out + int((w < 0).sum())
    assert n_in > 50000 and n_out > 50000


def expected_keys(case):
    seqs, ks, groups, jobs, want = case
    owns, others = [], []
    for (q0, nq, t0, nt), w in zip(jobs, want):
        o, x = crosstalk.reduce_distances(w, q0, groups[q0:q0 + nq], groups[t0:t0 + nt])
        owns.append(o)
        others.append(x)
    return np.concatenate(owns), np.concatenate(others)


@pytest.mark.parametrize("min_chunks", ["1", "18446744073709551615", None])
def test_keys_equal_the_host_reduction(case, monkeypatch, min_chunks):
    """One run per class (SMX_NEAREST_MIN_CHUNKS=1), runs of one ref (a huge value) and the library's own choice."""
    if min_chunks is None:
        monkeypatch.delenv("SMX_NEAREST_MIN_CHUNKS", raising=False)
    else:
        monkeypatch.setenv("SMX_NEAREST_MIN_CHUNKS", min_chunks)
    seqs, ks, groups, jobs, want = case
    own, other = crosstalk.nearest(seqs, ks, groups, jobs)
    want_own, want_other = expected_keys(case)
    assert own.shape == want_own.shape and (own == want_own).all() and (other == want_other).all()
    none = np.uint64(crosstalk.NONE)
    # every kind of read is there: both keys, one of them, neither; and ties at the winning distance go to the lower ref
    both = (own != none) & (other != none)
    assert both.sum() >= 20 and ((own != none) & (other == none)).sum() >= 20 and ((own == none) & (other != none)).sum() >= 20
    assert ((own == none) & (other == none)).sum() >= 20
    assert (own[-2:] == none).all() and (other[-2:] == none).all()     # the job without refs
    again = crosstalk.nearest(seqs, ks, groups, jobs)
    assert (again[0] == own).all() and (again[1] == other).all()      # two calls give identical arrays


def test_argument_errors_carry_a_message():
    lib = _lib.load()
    seqs = [b"ACGTACGT", b"ACGAACGT", b"", b"ACGT", b"ACGTT"]
    off = calls.offsets(seqs)
    ks = np.array([2] * len(seqs), dtype=np.int32)
    group = np.arange(len(seqs), dtype=np.uint32)

    def call(jobs):
        jarr = np.array(jobs, dtype=_lib.NEAREST_JOB_DTYPE)
        a, b = np.zeros(64, dtype=np.uint64), np.zeros(64, dtype=np.uint64)
        rc = lib.smx_nearest(b"".join(seqs), _lib.ptr(off), len(seqs), _lib.ptr(ks), _lib.ptr(group), _lib.ptr(jarr), len(jobs),
                             _lib.ptr(a), _lib.ptr(b), None)
        return rc, lib.smx_last_error().decode(), a, b
    for jobs, word in (([(1, 2, 3, 2)], "empty ref"), ([(0, 6, 3, 1)], "out of bounds"), ([(0, 1, 4, 2)], "out of bounds"),
                       ([(0, 2, 2, 2), (0, 1, 3, 2)], "overlap")):
        rc, msg, _, _ = call(jobs)
        assert rc == _lib.ERR_ARG and word in msg, (jobs, rc, msg)
    rc, msg, a, b = call([(0, 2, 2, 1), (0, 1, 3, 2)])             # an empty read, shared refs: good
    assert rc == _lib.OK, msg
    none = crosstalk.NONE
    # the empty read (group 2, limit 2) is 8 from both refs: no key.  ACGT and ACGTT against ACGTACGT: 4 and 3, above the limit
    assert [int(x) for x in a[:3]] == [none] * 3 and [int(x) for x in b[:3]] == [none] * 3
