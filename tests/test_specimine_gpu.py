"""specimine on the GPU: the mining kernel's HW distances against the O(m*n) oracle DP, and whole .mined files
against a plain-Python restatement of the reference loop (specimine.py:197-257) over oracle distances."""
import glob
import os
import random
import shutil

import numpy as np
import pytest

from conftest import GOLDEN
from oracle.edlib_semantics import HW, align_c
from specimux_amd import _lib, calls, specimine, synth

pytestmark = pytest.mark.gpu


def oracle_dist(q, t, k):
    return align_c(q, t, HW, k, iupac=False)["editDistance"]


def kernel_dists(pairs):
    """[(query, target, k)] -> kernel distances, one smx_mine_distances call (one job per pair group of a query/k)."""
    lib = _lib.load()
    groups = {}
    for i, (q, t, k) in enumerate(pairs):
        groups.setdefault((q, k), []).append(i)
    queries, ks, targets, jobs, order = [], [], [], [], []
    for (q, k), idx in groups.items():
        jobs.append((len(queries), 1, len(targets), len(idx), 0.0))
        queries.append(q.encode("latin-1"))
        ks.append(k)
        targets.extend(pairs[i][1].encode("latin-1") for i in idx)
        order.extend(idx)
    qoff, toff = calls.offsets(queries), calls.offsets(targets)
    jarr = np.array(jobs, dtype=_lib.MINE_JOB_DTYPE)
    dist = np.full(len(pairs), -7, dtype=np.int32)
    _lib.check(lib.smx_mine_distances(b"".join(queries), _lib.ptr(qoff), len(queries), _lib.ptr(np.array(ks, np.int32)),
                                      b"".join(targets), _lib.ptr(toff), len(targets), _lib.ptr(jarr), len(jobs),
                                      _lib.ptr(dist), None))
    out = np.empty(len(pairs), dtype=np.int64)
    out[np.array(order)] = dist
    return out


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, rate, alphabet="ACGT"):
    out = []
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            out.append(rng.choice(alphabet))
        elif r < 2 * rate / 3:
            out.append(ch + rng.choice(alphabet))
        elif r >= rate:
            out.append(ch)
    return "".join(out)


def check(pairs):
    got = kernel_dists(pairs)
    bad = [(len(q), len(t), k, int(g), oracle_dist(q, t, k)) for (q, t, k), g in zip(pairs, got)
           if g != oracle_dist(q, t, k)]
    assert not bad, f"{len(bad)} of {len(pairs)} pairs differ (m, n, k, kernel, oracle): {bad[:10]}"


def test_distances_lengths_and_limits():
    rng = random.Random(11)
    pairs = []
    for m in (1, 2, 63, 64, 65, 127, 128, 129, 200, 600, 1025, 1500, 4097, 5000):
        ks = sorted({0, min(3, m), int(0.15 * m), m, m + 5, -1})
        reps = 6 if m <= 1500 else 1
        for _ in range(reps):
            alphabet = rng.choice(["ACGT", "ACGT", "ACGTNRY", "ACGTacgtN"])
            q = rand_seq(rng, m, alphabet)
            for k in ks:
                kk = m if k < 0 else k
                core = mutate(rng, q, 0.1, alphabet)
                cands = [
                    core,                                                                   # about m
                    q,                                                                      # identical
                    core[:max(0, m - kk - 1 - rng.randrange(3))],                           # shorter than m - k
                    rand_seq(rng, rng.randrange(0, 40)) + core + rand_seq(rng, rng.randrange(0, 40)),
                    "",                                                                     # empty target
                ]
                if m <= 1500:
                    cands.append(rand_seq(rng, rng.randrange(m, 2 * m + 40)) + core + rand_seq(rng, m // 2))  # much longer
                    cands.append(rand_seq(rng, m + rng.randrange(-3, 30), alphabet))          # unrelated
                for t in cands:
                    pairs.append((q, t, k))
    assert len(pairs) > 1000
    check(pairs)


def test_distances_long_query():
    rng = random.Random(12)
    q = rand_seq(rng, 16400)
    t = rand_seq(rng, 50) + mutate(rng, q, 0.05) + rand_seq(rng, 50)
    check([(q, t, int(0.15 * len(q))), (q, t, 10)])


def test_distances_one_query_many_targets_and_many_queries_one_target():
    rng = random.Random(13)
    q = rand_seq(rng, 300)
    targets = [mutate(rng, q, rng.uniform(0, 0.3)) if i % 3 else rand_seq(rng, rng.randrange(250, 350))
               for i in range(1000)]
    check([(q, t, 45) for t in targets])
    t = rand_seq(rng, 400)
    queries = [mutate(rng, t[s:s + ln], 0.1) or "A" for s, ln in ((rng.randrange(0, 250), rng.randrange(1, 150)) for _ in range(1000))]
    check([(x, t, int(len(x) * 0.15)) for x in queries])


def test_distances_walk_over_many_short_records():
    """The chunk walk (smx_mine_lds.h) where it can go wrong, all in state class 1: more than 4096 (job, query) records, so
    that the owner search takes its third round; records of one, two and three chunks in turn, so that most workgroups
    of 8 chunks start inside a record; a chunk total that is no multiple of 8.  The sequences are drawn from two small
    pools, so the oracle aligns every distinct pair once; every distance of the call is compared."""
    rng = random.Random(14)
    qpool = [rand_seq(rng, rng.randrange(12, 41)) for _ in range(48)]
    kpool = [rng.choice((-1, 2, 5, 9)) for _ in qpool]
    tpool = [rand_seq(rng, rng.randrange(12, 41)) if i % 2 else mutate(rng, qpool[i], 0.15)[:40].ljust(12, "A")
             for i in range(48)]
    table = np.array([[oracle_dist(q, t, k) for t in tpool] for q, k in zip(qpool, kpool)], dtype=np.int64)
    n_rec = 4201
    qid = [rng.randrange(48) for _ in range(n_rec)]
    tid = np.array([rng.randrange(48) for _ in range(600)])
    jobs = [(i, 1, rng.randrange(300), (1, 129, 257)[i % 3], 0.0) for i in range(n_rec)]
    starts = np.concatenate([[0], np.cumsum([(j[3] + 127) // 128 for j in jobs])])      # the records' chunk prefix
    first = np.arange(0, starts[-1], 8)                                                # every workgroup's first chunk
    assert starts[-1] % 8 != 0 and np.isin(first, starts, invert=True).mean() > 0.5
    want = np.concatenate([table[qid[i], tid[t0:t0 + nt]] for i, _, t0, nt, _ in jobs])
    assert (want >= 0).sum() > 50000 and (want == -1).sum() > 50000
    rc, got = mine_raw([qpool[x] for x in qid], [kpool[x] for x in qid], [tpool[x] for x in tid], jobs)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    bad = np.nonzero(got != want)[0]
    assert got.size == want.size > 500000 and bad.size == 0, \
        f"{bad.size} of {got.size} distances differ: {[(int(x), int(got[x]), int(want[x])) for x in bad[:10]]}"


# ---------------------------------------------------------------------------------------- edges of the kernel
ALL_BYTES = "".join(map(chr, range(256)))


def mine_raw(queries, ks, targets, jobs, best=False, sentinel=None):
    """One smx_mine_distances (best=False) or smx_mine_best_identity call on str/bytes sequences; jobs are
    (q0, nq, t0, nt, min_identity).  The output is filled with a sentinel first.  -> (status, output array)."""
    lib = _lib.load()
    qs = [q.encode("latin-1") if isinstance(q, str) else q for q in queries]
    ts = [t.encode("latin-1") if isinstance(t, str) else t for t in targets]
    qoff, toff = calls.offsets(qs), calls.offsets(ts)
    jarr = np.array(jobs, dtype=_lib.MINE_JOB_DTYPE)
    if best:
        n_out = sum(j[3] for j in jobs)
        out = np.full(max(n_out, 1), -5.0 if sentinel is None else sentinel, dtype=np.float64)
        fn = lib.smx_mine_best_identity
    else:
        n_out = sum(j[1] * j[3] for j in jobs)
        out = np.full(max(n_out, 1), -7 if sentinel is None else sentinel, dtype=np.int32)
        fn = lib.smx_mine_distances
    rc = fn(b"".join(qs), _lib.ptr(qoff), len(qs), _lib.ptr(np.array(ks, dtype=np.int32)), b"".join(ts), _lib.ptr(toff),
            len(ts), _lib.ptr(jarr), len(jobs), _lib.ptr(out), None)
    return rc, out[:n_out]


def expected_dists(queries, ks, targets, jobs):
    """The oracle's distances in smx_mine_distances' layout (per job, row-major over its queries x targets)."""
    out = []
    for q0, nq, t0, nt, _ in jobs:
        for i in range(q0, q0 + nq):
            out.extend(oracle_dist(queries[i], targets[t], ks[i]) for t in range(t0, t0 + nt))
    return np.array(out, dtype=np.int64)


def assert_oracle(pairs, got):
    bad = [(len(q), len(t), k, int(g), w) for (q, t, k), g in zip(pairs, got) if g != (w := oracle_dist(q, t, k))]
    assert not bad, f"{len(bad)} of {len(pairs)} pairs differ (m, n, k, kernel, oracle): {bad[:10]}"


def band_targets(rng, q, alphabet="ACGT"):
    """Targets that put the band's edges to work: point edits, edits on block rows / columns 63/64, 127/128, ...,
    one long insertion or deletion (64-300 nt), a tandem repeat of a piece of the query, and the query flanked."""
    m = len(q)
    out = [mutate(rng, q, rng.uniform(0.005, 0.12), alphabet)]
    t = list(q)
    for p in range(((m - 1) // 64) * 64, -1, -64):
        for pos in (p, p - 1):
            if pos < 0 or pos >= len(t) or rng.random() < 0.4:
                continue
            op = rng.randrange(3)
            if op == 0:
                t[pos] = rng.choice(alphabet)
            elif op == 1:
                t.insert(pos, rng.choice(alphabet))
            else:
                del t[pos]
    out.append("".join(t))
    ln = rng.randrange(64, 301)
    base = mutate(rng, q, 0.02, alphabet)
    pos = rng.randrange(len(base) + 1)
    out.append(base[:pos] + rand_seq(rng, ln, alphabet) + base[pos:])
    if m > ln + 16:
        pos = rng.randrange(m - ln)
        out.append(mutate(rng, q[:pos] + q[pos + ln:], 0.02, alphabet))
    ul = rng.randrange(1, min(m, 70) + 1)
    s0 = rng.randrange(m - ul + 1)
    out.append(mutate(rng, (q[s0:s0 + ul] * (m // ul + 2))[:m + rng.randrange(-m // 4, m // 4 + 64)], 0.03, alphabet))
    out.append(rand_seq(rng, rng.randrange(0, 120), alphabet) + mutate(rng, q, 0.05, alphabet) +
               rand_seq(rng, rng.randrange(0, 120), alphabet))
    return out


def test_band_at_class_boundaries():
    """k at the distance (d - 1, d, d + 1) at every register-class edge and beyond, with long indels and edits on
    block boundaries: the three band rules act exactly between d <= k and d > k."""
    rng = random.Random(21)
    pairs, at = [], {-1: 0, 0: 0, 1: 0}
    for m in (64, 65, 256, 257, 512, 513, 1023, 1024, 1025, 2049):
        for rep in range(2):
            alphabet = "ACGT" if rep == 0 else "AC"
            q = rand_seq(rng, m, alphabet)
            if rep == 1:   # a tandem-repeat query
                unit = rand_seq(rng, rng.randrange(2, 40), alphabet)
                q = mutate(rng, (unit * (m // len(unit) + 1))[:m], 0.02, alphabet)[:m].ljust(m, "A")
            for t in band_targets(rng, q, alphabet):
                d = oracle_dist(q, t, -1)
                for dk in (-1, 0, 1):
                    if d + dk >= 0:
                        pairs.append((q, t, d + dk))
                        at[dk] += 1
    assert min(at.values()) >= 100 and len({len(q) for q, _, _ in pairs}) == 10
    assert_oracle(pairs, kernel_dists(pairs))


def test_generic_class_grid_stride():
    """More class-0 chunks than MINE_BLOCK_CHUNKS times the grid cap, so that the cap binds and workgroups take longer
    runs: each one rebuilds its LDS Peq for queries of other lengths and reuses its scratch slice."""
    rng = random.Random(22)
    long_q = rand_seq(rng, 130972)
    # smx_chunk_plan.h, chunk_scratch_cap and chunk_grid: cap = 256 MiB / slice, slice = 3 * W_max * MINE_THREADS * 8
    # bytes; per_block = max(MINE_BLOCK_CHUNKS, ceil(chunks / cap)), one chunk per query here (1-3 targets each)
    w_max = (len(long_q) + 63) // 64
    cap = (256 << 20) // (3 * w_max * 128 * 8)
    assert 40 <= cap <= 45
    queries, ks, targets, jobs = [], [], [], []
    n_q = 10 * cap + 30
    for i in range(n_q):
        if i == n_q // 2:   # short targets: the oracle's O(m n) stays cheap; k = -1 runs all 2047 words of the band
            s0 = rng.randrange(len(long_q) - 400)
            q, tl = long_q, [rand_seq(rng, 40) + mutate(rng, long_q[s0:s0 + 300], 0.05), long_q[s0:s0 + 400]]
            k = -1
        else:
            q = rand_seq(rng, rng.randrange(1025, 1401))
            tl = [mutate(rng, q, rng.uniform(0.02, 0.12)) for _ in range(rng.randrange(1, 4))]
            if rng.random() < 0.3:
                tl[-1] = rand_seq(rng, rng.randrange(0, 30)) + tl[-1] + rand_seq(rng, rng.randrange(0, 30))
            k = rng.choice([int(0.15 * len(q)), -1, int(0.08 * len(q)), 40])
        jobs.append((len(queries), 1, len(targets), len(tl), 0.0))
        queries.append(q)
        ks.append(k)
        targets.extend(tl)
    n_chunks = len(queries)   # every query has 1-3 targets: one chunk each, all in the generic class (W > 16)
    per_block = max(8, -(-n_chunks // cap))
    assert all((len(q) + 63) // 64 > 16 for q in queries) and per_block > 8
    assert len({(len(q) + 63) // 64 for q in queries}) >= 5
    rc, got = mine_raw(queries, ks, targets, jobs)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    want = expected_dists(queries, ks, targets, jobs)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} of {got.size} distances differ: {[(int(got[i]), int(want[i])) for i in bad[:10]]}"
    assert (want >= 0).sum() > len(targets) // 2


def lds_table_bytes(m, rows):
    """LDS bytes of a query's Peq table (smx_chunk_plan.h, chunk_table): MINE_LDS_HEAD words + (rows + 1) x (W | 1) words."""
    return (192 + (rows + 1) * (((m + 63) // 64) | 1)) * 8


def all_bytes_query(rng, m):
    q = list(ALL_BYTES) + [rng.choice(ALL_BYTES) for _ in range(m - 256)]
    rng.shuffle(q)
    return "".join(q)


def test_bytes_0x00_to_0xff():
    rng = random.Random(23)
    pairs = []
    for m in (1, 5, 64, 100, 300, 700, 1100):
        for _ in range(3):
            q = rand_seq(rng, m, ALL_BYTES)
            for t in (mutate(rng, q, 0.08, ALL_BYTES), rand_seq(rng, 20, ALL_BYTES) + mutate(rng, q, 0.04, ALL_BYTES),
                      rand_seq(rng, m + 10, ALL_BYTES), q.replace(q[0], "\x00")):
                d = oracle_dist(q, t, -1)
                pairs.extend((q, t, k) for k in {-1, max(d - 1, 0), d, int(0.15 * m)})
    seen_q = set("".join(q for q, _, _ in pairs))
    seen_t = set("".join(t for _, t, _ in pairs))
    assert "\x00" in seen_q and "\x00" in seen_t and len(seen_q & seen_t & set(ALL_BYTES[0x80:])) >= 120
    assert_oracle(pairs, kernel_dists(pairs))


def test_256_distinct_bytes_table_above_64k():
    rng = random.Random(24)
    q = all_bytes_query(rng, 2048)
    assert len(set(q)) == 256 and lds_table_bytes(len(q), 256) == 69384 > 65536   # the hipFuncSetAttribute path
    targets = [mutate(rng, q, 0.05, ALL_BYTES), rand_seq(rng, 50, ALL_BYTES) + mutate(rng, q[300:1900], 0.03, ALL_BYTES),
               rand_seq(rng, 2100, ALL_BYTES)]
    pairs = []
    for t in targets:
        d = oracle_dist(q, t, -1)
        pairs.extend((q, t, k) for k in (-1, d - 1, d, d + 1, int(0.15 * len(q))))
    assert_oracle(pairs, kernel_dists(pairs))


def test_lds_limit_at_its_edge():
    """SMX_LDS_POOL = 159744 bytes: 256 distinct bytes fit at m = 4800 (W = 75) and not at m = 4864 (W = 76, Wp = 77)."""
    rng = random.Random(25)
    fits, over = all_bytes_query(rng, 4800), all_bytes_query(rng, 4864)
    assert lds_table_bytes(4800, 256) == 155736 <= 159744 < lds_table_bytes(4864, 256) == 159848
    t = mutate(rng, fits, 0.04, ALL_BYTES)
    d = oracle_dist(fits, t, -1)
    pairs = [(fits, t, -1), (fits, t, d), (fits, t, d - 1)]
    assert_oracle(pairs, kernel_dists(pairs))
    rc, _ = mine_raw([over], [-1], [mutate(rng, over, 0.04, ALL_BYTES)], [(0, 1, 0, 1, 0.0)])
    msg = _lib.load().smx_last_error().decode()
    assert rc == _lib.ERR_UNSUPPORTED and "do not fit the LDS" in msg and "159848 > 159744" in msg, (rc, msg)
    pairs = [(fits[:700], t[:760], 100), (fits[:3000], t, -1)]   # the next call is unaffected
    assert_oracle(pairs, kernel_dists(pairs))


def reference_best(queries, ks, targets, jobs, dist_of):
    """The reference's loop (specimine.py:197-257) per (job, target): best starts at 0 and only grows; d != -1,
    identity >= min_identity; identity = 1 - d / m in IEEE double."""
    out = []
    for q0, nq, t0, nt, mi in jobs:
        for t in range(t0, t0 + nt):
            b = 0.0
            for i in range(q0, q0 + nq):
                d = dist_of(i, t)
                if d == -1:
                    continue
                identity = 1 - d / len(queries[i])
                if identity >= mi and identity > b:
                    b = identity
            out.append(b)
    return np.array(out, dtype=np.float64)


def test_best_identity_direct():
    rng = random.Random(26)
    queries, ks, targets = [], [], []
    base = [rand_seq(rng, rng.randrange(40, 160)) for _ in range(30)]   # a few families: many pairs score well
    for _ in range(400):
        src = rng.choice(base)
        queries.append(mutate(rng, src, rng.uniform(0, 0.1)))
        m = len(queries[-1])
        ks.append(rng.choice([-1, m, int(0.1 * m), int(0.25 * m), rng.randrange(0, m + 1)]))   # k apart from min_identity
    for _ in range(900):
        targets.append(mutate(rng, rng.choice(base), rng.uniform(0, 0.2)) if rng.random() < 0.85
                       else rand_seq(rng, rng.randrange(0, 200)))
    cache = {}

    def dist_of(i, t):
        if (i, t) not in cache:
            cache[(i, t)] = oracle_dist(queries[i], targets[t], ks[i])
        return cache[(i, t)]

    jobs = [(0, 0, 0, 5, 0.5), (3, 2, 10, 0, 0.5), (7, 0, 900, 0, 0.0)]   # empty jobs at the start
    # wide jobs: nq up to 40 queries x up to 300 targets (several work items per query), target ranges overlapping
    jobs += [(0, 40, 0, 300, 0.8), (20, 30, 150, 290, 0.7), (200, 12, 500, 140, 0.0)]
    n_exact = 0
    while len(jobs) < 1100:
        if len(jobs) == 550:
            jobs += [(5, 0, 100, 7, 0.9), (8, 3, 40, 0, 0.9), (0, 0, 0, 0, 0.9)]   # empty jobs in the middle
        q0, t0 = rng.randrange(400), rng.randrange(900)
        nq, nt = rng.randint(1, min(4, 400 - q0)), rng.randint(1, min(4, 900 - t0))
        mi = rng.choice([0.0, 0.5, 0.8, 0.85, 0.9, 0.95, 1.0])
        if rng.random() < 0.35:   # min_identity exactly at one of the job's identities, or one ulp on either side
            found = [1 - d / len(queries[i]) for i in range(q0, q0 + nq) for t in range(t0, t0 + nt)
                     if (d := dist_of(i, t)) != -1]
            if found:
                mi = float(np.nextafter(rng.choice(found), rng.choice([0.0, 2.0]))) if rng.random() < 0.6 else rng.choice(found)
                n_exact += 1
        jobs.append((q0, nq, t0, nt, mi))
    jobs += [(399, 1, 899, 0, 0.5), (0, 0, 899, 1, 0.5)]   # empty jobs at the end
    assert len(jobs) >= 1000 and n_exact >= 100
    want = reference_best(queries, ks, targets, jobs, dist_of)
    rc, got = mine_raw(queries, ks, targets, jobs, best=True)
    assert rc == _lib.OK, _lib.load().smx_last_error()
    assert got.shape == want.shape
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]   # bit for bit, not approximately
    assert bad.size == 0, f"{bad.size} of {got.size} differ: {[(float(got[i]), float(want[i])) for i in bad[:10]]}"
    # the thresholds and limits decided something: exact-threshold hits, -1 skips, zero and nonzero results
    assert (want > 0).sum() > 500 and (want == 0).sum() > 100
    assert sum(d == -1 for d in cache.values()) > 500


def test_workspace_reuse_and_every_slot_written():
    """Large, small, large again in one process, with the outputs filled with a sentinel first: the grow-only device
    workspace must not leak one call's data into the next, and every output slot must be written."""
    rng = random.Random(27)
    queries, ks, targets, jobs = [], [], [], []
    for m in [20, 64, 100, 128, 200, 300, 500, 700, 1000, 1300, 2100]:
        q = rand_seq(rng, m)
        tl = [rng.choice(band_targets(rng, q)) for _ in range(rng.choice([1, 60, 130]))]
        jobs.append((len(queries), 1, len(targets), len(tl), 0.0))
        queries.append(q)
        ks.append(int(0.15 * m))
        targets.extend(tl)
    jobs.append((0, len(queries), 0, 40, 0.7))   # every query against the first 40 targets as well
    big = (queries, ks, targets, jobs)
    small = (["ACGTACGTAC"], [2], ["TTACGTTCGTACAA", "", "ACG"], [(0, 1, 0, 3, 0.0)])
    want = {id(big): expected_dists(*big), id(small): expected_dists(*small)}
    for call in (big, small, big):
        for sentinel in (-7, 123456):
            rc, got = mine_raw(*call, sentinel=sentinel)
            assert rc == _lib.OK, _lib.load().smx_last_error()
            assert np.array_equal(got, want[id(call)])
    cache = {}

    def dist_of(call, i, t):
        if (id(call), i, t) not in cache:
            cache[(id(call), i, t)] = oracle_dist(call[0][i], call[2][t], call[1][i])
        return cache[(id(call), i, t)]

    for call in (big, small, big):
        wbest = reference_best(*call, lambda i, t: dist_of(call, i, t))
        for sentinel in (-5.0, np.nan):
            rc, got = mine_raw(*call, best=True, sentinel=sentinel)
            assert rc == _lib.OK, _lib.load().smx_last_error()
            assert np.array_equal(got.view(np.uint64), wbest.view(np.uint64))


def test_argument_errors_leave_the_next_call_correct():
    rng = random.Random(28)
    q = rand_seq(rng, 150)
    t = mutate(rng, q, 0.05)
    good = ([q], [30], [t, q[10:140]], [(0, 1, 0, 2, 0.0)])
    want = expected_dists(*good)
    lib = _lib.load()
    for best in (False, True):
        rc, _ = mine_raw([q, ""], [30, 30], [t], [(0, 1, 0, 1, 0.0)], best=best)         # an empty query
        assert rc == _lib.ERR_ARG and "empty" in lib.smx_last_error().decode()
        rc, _ = mine_raw(*good, best=best)
        assert rc == _lib.OK
        rc, _ = mine_raw([q], [30], [t, t], [(0, 1, 1, 2, 0.0)], best=best)               # targets 1..2 of 2
        assert rc == _lib.ERR_ARG and "out of bounds" in lib.smx_last_error().decode()
        rc, got = mine_raw(*good)
        assert rc == _lib.OK and np.array_equal(got, want)
        rc, got = mine_raw([q], [30], [t], [], best=best)                                  # no jobs at all
        assert rc == _lib.OK and got.size == 0


# ---------------------------------------------------------------------------------------- whole files
def expected_mined_text(index, fastq, partial_forward, no_partial_reverse, min_identity):
    """The reference's mining loop restated over oracle distances, formatted as its FASTQ writer does."""
    sid = specimine.extract_specimen_id(fastq)
    b1, b2 = specimine.find_barcodes(sid, index)
    files = specimine.derive_partial_match_filenames(fastq, b1, b2)
    if not partial_forward:
        files.pop("forward", None)
    if no_partial_reverse:
        files.pop("reverse", None)
    fulls = specimine.read_fastq(fastq)
    out = []
    if not fulls:
        return ""
    for ptype, flist in files.items():
        for f in flist:
            for p in specimine.read_fastq(f):
                best = 0
                for fr in fulls:
                    k = int(len(fr.seq) * (1 - min_identity))
                    d = oracle_dist(fr.seq, p.seq, k)
                    if d != -1:
                        identity = 1 - (d / len(fr.seq))
                        if identity >= min_identity and identity > best:
                            best = identity
                if best:
                    title = f"{p.id}_mined_{ptype}_{best:.2f} {p.description} mined_{ptype} identity={best:.2f}"
                    out.append(f"@{title}\n{p.seq}\n+\n{p.quality_string}\n")
    return "".join(out)


def run_cli(fastq, index, partial_forward, no_partial_reverse, min_identity):
    argv = ["--index", index, "--fastq", fastq, "--min-identity", repr(min_identity)]
    if partial_forward:
        argv.append("--partial-forward")
    if no_partial_reverse:
        argv.append("--no-partial-reverse")
    specimine.main(argv)
    with open(fastq + ".mined", encoding="latin-1") as fh:
        return fh.read()


@pytest.mark.parametrize("min_identity", [0.85, 0.3])
def test_golden_tree_pool_level(tmp_path, monkeypatch, min_identity):
    shutil.copytree(os.path.join(GOLDEN, "expected_output"), tmp_path / "out")
    shutil.copy(os.path.join(GOLDEN, "specimens.txt"), tmp_path / "out" / "specimens.txt")
    monkeypatch.chdir(tmp_path / "out")
    fastq = "full/ITS2/TEST_SPECIMEN_001.fastq"
    files = specimine.derive_partial_match_filenames(fastq, "ATAATATTCGGCA", "AACGGCCTTGAGG")
    assert sorted(os.path.basename(os.path.dirname(f)) for f in files["forward"]) == ["gITS7-ITS4", "gITS7-unknown"]
    got = run_cli(fastq, "specimens.txt", True, False, min_identity)
    assert got == expected_mined_text("specimens.txt", fastq, True, False, min_identity)
    if min_identity < 0.5:
        assert got.count("\n+\n") > 0, "the low threshold should mine something"


def test_synthetic_tree(tmp_path):
    root = str(tmp_path)
    ids = synth.write_mine_tree(root, n_specimens=3, n_full=5, n_partial=12, length=300, seed=5,
                                pairs=("P1-P2", "P1-P3"))
    # ties between full reads of different length: a full file whose reads are one insert and its 1-nt-shorter prefix
    with open(os.path.join(root, "full", "POOL", ids[0] + ".fastq")) as fh:
        lines = fh.read().split("\n")
    s = lines[1]
    with open(os.path.join(root, "full", "POOL", ids[0] + ".fastq"), "a") as fh:
        fh.write(f"@tie_a\n{s[:-1]}\n+\n{'I' * (len(s) - 1)}\n@tie_b\n{s[:-2]}\n+\n{'I' * (len(s) - 2)}\n")
    index = os.path.join(root, "specimens.txt")
    total = 0
    for sid in ids:
        for fastq in (os.path.join(root, "full", "POOL", f"{sid}.fastq"), os.path.join(root, "full", "POOL", "P1-P2", f"{sid}.fastq")):
            for min_identity in (0.0, 0.5, 0.85, 1.0):
                for pf, npr in ((True, False), (False, False), (True, True)):
                    got = run_cli(fastq, index, pf, npr, min_identity)
                    assert got == expected_mined_text(index, fastq, pf, npr, min_identity), (fastq, min_identity, pf, npr)
                    total += got.count("\n+\n")
    assert total > 0


def test_mine_specimens_equals_one_run_per_specimen(tmp_path):
    root = str(tmp_path)
    ids = synth.write_mine_tree(root, n_specimens=6, n_full=4, n_partial=10, length=250, seed=9)
    index = os.path.join(root, "specimens.txt")
    fastqs = [os.path.join(root, "full", "POOL", f"{sid}.fastq") for sid in ids]
    single = {}
    for f in fastqs:
        single[f] = run_cli(f, index, True, False, 0.8)
        os.remove(f + ".mined")
    jobs = [specimine.plan_job(index, f, True, False, 0.8) for f in fastqs]
    for job in jobs:
        mined = specimine.mine_sequences(job.fastq, job.partial_files, 0.8)
        assert "".join(specimine.format_record(title, rec) for title, rec in mined) == single[job.fastq]
    specimine.mine_specimens(jobs)
    for f in fastqs:
        with open(f + ".mined", encoding="latin-1") as fh:
            assert fh.read() == single[f]
    assert sum(v.count("\n+\n") for v in single.values()) > 0
    assert glob.glob(os.path.join(root, "full", "POOL", "*.mined"))
