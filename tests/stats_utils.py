"""Helpers of the specimux-stats tests (test_stats_cpu.py, test_stats_gpu.py): the oracle's trace as a stats table, and
the oracle's hit tables and primary records in the binary layout the statistics kernel reads (tests/cpu/stats_sim.cpp).
Behind them, for test_stats_kernel_gpu.py and its CPU runs in test_stats_cpu.py: synthetic hit tables that steer the
kernel to its edges (case_*) and rows_reference, the table such records must give, written from the rows' definition."""
import json
import os
import types

import numpy as np

from oracle import specimux_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_GOLDEN = os.path.join(REPO, "tests", "golden", "stats")
QUERIES = json.load(open(os.path.join(STATS_GOLDEN, "queries.json")))
CASES = ["golden_default", "golden_n11_20", "golden_derep_none", "golden_no_preorient", "golden_min_length_600", "c2_synth"]


def queries_of(case):
    return [q for q in QUERIES if q["cases"] == "all" or case in q["cases"]]


def unpack_trace(case, tmp_path):
    """The case's trace.tsv.gz as a trace directory (one specimux_trace_*.tsv) under tmp_path."""
    import gzip
    d = tmp_path / f"trace_{case}"
    d.mkdir()
    with gzip.open(os.path.join(STATS_GOLDEN, case, "trace.tsv.gz"), "rb") as src:
        (d / "specimux_trace_fixture_main.tsv").write_bytes(src.read())
    return os.fspath(d)

# smx_hit / smx_op (include/smx.h), restated so that the CPU tests do not need the HIP library
HIT = np.dtype([("first_start", "<i4"), ("first_end", "<i4"), ("tail_end", "<i4"), ("pdist", "<i2"), ("nloc", "<i2"),
                ("bbest", "<i2"), ("ntied", "<i2"), ("first_tied", "<i2"), ("flags", "<i2")])
OP = np.dtype([("sample", "<i4"), ("trim_start", "<i4"), ("trim_end", "<i4"), ("pool", "<i2"), ("p1", "<i2"), ("p2", "<i2"),
               ("barcode", "<i2"), ("dist", "i1", (4,)), ("rtype", "u1"), ("flags", "u1"), ("n_ops", "<u2"), ("read", "<u4")])
OPF_TRIM_EMPTY = 2


def oracle_table(opanel, opar, reads):
    """(stats table the host aggregator builds from the oracle's level-1 trace of `reads`, the trace rows)."""
    from specimux_amd import trace_stats
    tr = O.Tracer(1, "main")
    ops, _t, _m = O.process_sequences(reads, opar, opanel, tr=tr, record_offset=1)
    O.trace_outputs(tr, ops)
    return trace_stats.table_from_rows(["t"] + row for row in tr.rows), tr.rows


def panel_view(opanel):
    """The index -> name tables of specimux_amd.panel.CompiledPanel (primer order, global barcode list, pair list with
    pools), built from the oracle's panel: what decode_key needs."""
    primers = list(opanel.primers.values())
    barcodes = []
    for p in primers:
        barcodes += [b for b in p.barcodes if b not in barcodes]
    pools, pairs = [], []
    pidx = {id(p): i for i, p in enumerate(primers)}
    for fp in opanel.get_primers(O.FWD):
        for rp in opanel.get_paired(fp.primer):
            pool = O.pool_from_primers(fp, rp)
            if pool is not None and pool not in pools:
                pools.append(pool)
            pairs.append((pidx[id(fp)], pidx[id(rp)], pools.index(pool) if pool is not None else -1))
    return types.SimpleNamespace(primers=primers, primer_names=[p.name for p in primers], barcodes=barcodes, pools=pools,
                                 pairs=pairs, pdir=[0 if p.direction == O.FWD else 1 for p in primers])


def sim_input(view, opanel, opar, reads):
    """Bytes of a stats_sim input: per read the oracle's search results as lean hit records and its primary record
    (rtype, n_ops, trim-empty flag) as the demux kernel would leave them.  Returns (bytes, ops, hits, per-barcode distances)."""
    NP = len(view.primers)
    prefilter = O.make_prefilter(opanel, opar) if opar.prefilter else None
    bidx = {b: i for i, b in enumerate(view.barcodes)}
    hits = np.zeros((len(reads), 2 * NP), dtype=HIT)
    bdist = np.full((len(reads), 2 * NP, max(len(p.barcodes) for p in view.primers)), -1, dtype=np.int8)
    ops = np.zeros(len(reads), dtype=OP)
    for i, rec in enumerate(reads):
        L = len(rec[1])
        ops["read"][i] = i
        if (opar.min_length != -1 and L < opar.min_length) or (opar.max_length != -1 and L > opar.max_length):
            continue   # rtype 0 = filtered
        table = O.hit_table(opar, opanel, rec, prefilter)
        s, rs = rec[1], O.revcomp(rec[1])
        for p, primer in enumerate(view.primers):
            k = opar.max_dist_primers[primer.primer]
            votes = (O.align_seq(primer.primer, s, k, 0, opar.search_len).matched(),
                     O.align_seq(primer.primer, rs, k, 0, opar.search_len).matched())
            for e, end in enumerate("AB"):
                h, t = hits[i, 2 * p + e], table[(primer.name, end)]
                h["pdist"], h["bbest"], h["first_tied"], h["flags"] = t["pdist"], -1, -1, int(votes[e])
                h["first_start"] = h["first_end"] = h["tail_end"] = -1
                if t["pdist"] >= 0:
                    h["nloc"], (h["first_start"], h["first_end"]) = len(t["locs"]), t["locs"][0]
                dists = {bc: d for bc, (d, _l) in t["barcodes"].items()}
                if t["pdist"] >= 0 and dists:
                    best = min(dists.values())
                    tied = [bc for bc in primer.barcodes if dists.get(bc) == best]
                    h["bbest"], h["ntied"], h["first_tied"] = best, len(tied), bidx[tied[0]]
                    h["tail_end"] = max(loc[1] for _d, locs in t["barcodes"].values() for loc in locs)
                    for bi, bc in enumerate(primer.barcodes):
                        bdist[i, 2 * p + e, bi] = dists.get(bc, -1)
        rops, _t, _m = O.process_sequences([rec], opar, opanel, prefilter)
        first = rops[0]
        ops["rtype"][i], ops["n_ops"][i] = first.rtype, len(rops)
        if (first.p1 == "unknown" and first.p1_loc is not None) or (first.p2 == "unknown" and first.p2_loc is not None):
            ops["flags"][i] |= OPF_TRIM_EMPTY    # the fallback record no longer names the primers its candidate matched
    return sim_bytes(NP, view.pdir, view.pairs, opar.preorient, hits, ops), ops, hits, bdist


def sim_bytes(NP, pdir, pairs, preorient, hits, ops):
    """A stats_sim input file (layout: tests/cpu/stats_sim.cpp) of hit records [n, 2 * NP] and primary records [n]."""
    assert hits.dtype == HIT and ops.dtype == OP and hits.shape == (len(ops), 2 * NP)
    head = np.array([NP, len(pairs), 1 if preorient else 0, len(ops)], dtype="<i4")
    body = [head, np.array(pdir, dtype="<i4"), np.array([p[0] for p in pairs], dtype="<i4"),
            np.array([p[1] for p in pairs], dtype="<i4")]
    return b"".join(a.tobytes() for a in body) + np.ascontiguousarray(hits).tobytes() + np.ascontiguousarray(ops).tobytes()


def parse_sim(text):
    """stdout of stats_sim -> (counters dict, fallback read indices, {key: count})."""
    counters, fallback, keys = {}, [], {}
    for line in text.splitlines():
        w = line.split()
        if w[0] == "counters":
            counters = {k: int(v) for k, v in (x.split("=") for x in w[1:])}
        elif w[0] == "fallback":
            fallback.append(int(w[1]))
        elif w[0] == "key":
            keys[int(w[1], 16)] = int(w[2])
    return counters, fallback, keys


# ------------------------------------------------------------------ synthetic hit tables: a reference of their own
# (tests/test_stats_kernel_gpu.py on the device, tests/test_stats_cpu.py through the CPU simulation)
R_FILTERED, R_FULL, R_PARTIAL_FWD, R_PARTIAL_REV, R_MULTIPLE, R_UNKNOWN, R_DEREP_FULL = range(7)    # SMX_R_* (include/smx.h)
OPF_REVERSE, OPF_NO_SPECIMEN = 1, 4
CLASS_UNKNOWN, CLASS_FULL, CLASS_PARTIAL_FWD, CLASS_PARTIAL_REV, CLASS_MULTIPLE, CLASS_DISCARDED = range(6)
THREADS, LCAP, LPROBE = 256, 2048, 16      # STATS_THREADS, STATS_LCAP, STATS_LPROBE (smx_stats_core.h), restated
FIRST = 1 << 45
_CLASS_OF_RTYPE = {R_FULL: CLASS_FULL, R_PARTIAL_FWD: CLASS_PARTIAL_FWD, R_PARTIAL_REV: CLASS_PARTIAL_REV,
                   R_MULTIPLE: CLASS_MULTIPLE}
# candidate score of the reference by (primers matched, barcodes matched); a barcode only counts beside its primer
_SCORE = {(2, 2): 5, (2, 1): 4, (1, 1): 3, (2, 0): 2, (1, 0): 1}


def pack_key(ori, pair1, p1, p2, b1, b2, cls, first):
    """include/smx.h, "Match statistics": orientation [0, 2), 1 + pair [2, 14), primers 14 and 15, 1 + barcode [16, 29)
    and [29, 42), class [42, 45), first candidate 45."""
    assert 0 <= ori < 3 and 0 <= pair1 < 4096 and 0 <= b1 < 8192 and 0 <= b2 < 8192 and 0 <= cls < 6
    return ori | pair1 << 2 | int(p1) << 14 | int(p2) << 15 | b1 << 16 | b2 << 29 | cls << 42 | int(first) << 45


def read_rows(pdir, pairs, preorient, pdist, bbest, tied, vote, rtype, oflags):
    """Rows of one read: its 2 * NP hit records as four lists, its primary record as (rtype, flags).  None: the read goes
    to the fallback list."""
    if rtype == R_FILTERED:
        return [FIRST]
    if oflags & OPF_TRIM_EMPTY:
        return None
    ori = 0
    if preorient:
        # a forward primer found at end A or a reverse primer found at end B says "forward"; the other two say "reverse"
        fwd = sum(vote[2 * p + d] & 1 for p, d in enumerate(pdir))
        rev = sum(vote[2 * p + 1 - d] & 1 for p, d in enumerate(pdir))
        ori = 1 if fwd and not rev else 2 if rev and not fwd else 0
    cands = []
    for n, pair in enumerate(pairs):
        for o in (0, 1):              # o = 0: the read as it is (forward primer at end A), o = 1: its reverse complement
            if ori == 2 - o:
                continue
            a, b = 2 * pair[0] + o, 2 * pair[1] + 1 - o
            p1, p2 = pdist[a] >= 0, pdist[b] >= 0
            if not (p1 or p2):
                continue
            has1, has2 = p1 and bbest[a] >= 0, p2 and bbest[b] >= 0
            cands.append((_SCORE[p1 + p2, has1 + has2],
                          (ori, n + 1, p1, p2, tied[a] + 1 if has1 else 0, tied[b] + 1 if has2 else 0)))
    if not cands:
        return [ori | FIRST]
    best = max(score for score, _f in cands)
    cls = _CLASS_OF_RTYPE.get(rtype, CLASS_UNKNOWN)
    return [pack_key(*fields, cls if score == best else CLASS_DISCARDED, at == 0) for at, (score, fields) in enumerate(cands)]


def rows_per_read(NP, pdir, pairs, preorient, hits, ops):
    """[read_rows of read i] for hit records [n, 2 * NP] and primary records [n]."""
    assert hits.shape == (len(ops), 2 * NP) and len(pdir) == NP
    pd, bb, ft = hits["pdist"].tolist(), hits["bbest"].tolist(), hits["first_tied"].tolist()
    vt, rt, fl = hits["flags"].tolist(), ops["rtype"].tolist(), ops["flags"].tolist()
    return [read_rows(pdir, pairs, preorient, pd[i], bb[i], ft[i], vt[i], rt[i], fl[i]) for i in range(len(ops))]


def rows_reference(NP, pdir, pairs, preorient, hits, ops):
    """(Counter {key: count}, sorted indices of the reads on the fallback list): the statistics table of synthetic hit
    records and primary records, from the definition of the rows (include/smx.h "Match statistics", the reference's
    candidate score and orientation vote) -- not from smx_stats_core.h and not through trace_stats._keys_of_read."""
    import collections
    table, fallback = collections.Counter(), []
    for i, rows in enumerate(rows_per_read(NP, pdir, pairs, preorient, hits, ops)):
        if rows is None:
            fallback.append(i)
        else:
            table.update(rows)
    return table, fallback


def stats_hash_np(keys):
    """stats_hash (smx_stats_core.h) restated: only ever used to CHOOSE keys with a wanted home slot."""
    keys = np.asarray(keys, dtype=np.uint64)
    keys = keys ^ (keys >> np.uint64(29))
    return (keys * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32)


def blank_reads(NP, n):
    """n reads without any hit, unfiltered, a single record each."""
    hits, ops = np.zeros((n, 2 * NP), dtype=HIT), np.zeros(n, dtype=OP)
    for name in ("first_start", "first_end", "tail_end", "pdist", "bbest", "first_tied"):
        hits[name] = -1
    ops["rtype"], ops["n_ops"], ops["read"] = R_UNKNOWN, 1, np.arange(n)
    return hits, ops


def one_row_reads(NP, pair, b1, b2, rtype=R_FULL):
    """Reads that give exactly one row each on a preoriented panel: the only vote sits on the forward primer's end A (ori =
    1, only o = 0 is tried), both primers of `pair` = (fw, rv, ...) match there, barcode fields b1[i], b2[i] (0 = no barcode
    hit, else first_tied = field - 1).  The indices need not exist in the panel: the kernel never looks them up."""
    b1, b2 = np.asarray(b1, dtype=np.int64), np.asarray(b2, dtype=np.int64)
    hits, ops = blank_reads(NP, len(b1))
    for col, field in ((2 * pair[0], b1), (2 * pair[1] + 1, b2)):
        hits["pdist"][:, col], hits["nloc"][:, col] = 0, 1
        hits["bbest"][:, col] = np.where(field > 0, 0, -1)
        hits["ntied"][:, col] = field > 0
        hits["first_tied"][:, col] = field - 1
    hits["flags"][:, 2 * pair[0]] = 1
    ops["rtype"] = rtype
    return hits, ops


def one_row_key(pair1, b1, b2, cls=CLASS_FULL):
    """The key one_row_reads aims at (numpy): for choosing inputs by home slot, never an expected value."""
    b1, b2 = np.asarray(b1, dtype=np.uint64), np.asarray(b2, dtype=np.uint64)
    return np.uint64(pack_key(1, pair1, 1, 1, 0, 0, cls, 1)) | b1 << np.uint64(16) | b2 << np.uint64(29)


def keys_with_home(pair1, mask, home, want):
    """(b1, b2) of `want` distinct one-row keys of pair `pair1` whose hash & mask == home."""
    b1, b2 = [a.reshape(-1) for a in np.meshgrid(np.arange(1, 8191), np.arange(1, 61), indexing="ij")]
    at = np.flatnonzero((stats_hash_np(one_row_key(pair1, b1, b2)) & np.uint64(mask)) == np.uint64(home))[:want]
    assert len(at) == want
    return b1[at], b2[at]


def panel_nine_pairs():
    """The eight primers of synth.panel_c3 with five more pools that pair forward primers with other pools' reverse primers:
    nine pairs (primers pair when they share a specimen), most primers in several of them, so that random hits give many
    candidates per read.  An 8 x 6 barcode grid per pool keeps the panel small."""
    from specimux_amd import synth
    seq = {name: s for _pool, fn, fs, rn, rs in synth.POOLS_C3 for name, s in ((fn, fs), (rn, rs))}
    cross = [("ITS_LR5", "ITS1F", "LR5"), ("ITS_RPB2", "ITS1F", "RPB2-7.1R"), ("RPB2_ITS4", "fRPB2-5F", "ITS4"),
             ("LSU_ITS4", "LR0R", "ITS4"), ("TEF1_LR5", "EF1-983F", "LR5")]
    f, r = synth.make_barcodes(8, 6, seed=2002)
    return synth.Panel(list(synth.POOLS_C3) + [(pool, fn, seq[fn], rn, seq[rn]) for pool, fn, rn in cross], f, r)


# ---- the cases (A .. G of tests/test_stats_kernel_gpu.py); all of them deterministic
_HIT_STATES = [(pd, bb, v) for pd in (-1, 1) for bb in (-2, -1, 1) for v in (0, 1)]     # primer x barcode x vote
_OP_FLAGS = [0, OPF_REVERSE, OPF_NO_SPECIMEN, OPF_TRIM_EMPTY, OPF_TRIM_EMPTY | OPF_REVERSE]


def case_truth_table():
    """A (two primers): each of the four hit records in each of its 12 states, every hit row with every rtype 0..6; the
    record flags cycle with period 5, co-prime to 7, so that every rtype meets every flag."""
    NP = 2
    state = np.array(np.unravel_index(np.arange(12 ** 4), (12,) * 4)).T          # [20736, 4]
    hits, ops = blank_reads(NP, 12 ** 4 * 7)
    st = np.array(_HIT_STATES)[np.repeat(state, 7, axis=0)]                       # [n, 4, 3]
    hits["pdist"], hits["bbest"], hits["flags"] = st[:, :, 0], st[:, :, 1], st[:, :, 2]
    hits["first_tied"] = np.where(st[:, :, 1] >= 0, 3 + np.arange(4)[None, :], -1)   # a barcode of its own per record
    ops["rtype"] = np.tile(np.arange(7), 12 ** 4)
    ops["flags"] = np.array(_OP_FLAGS)[np.arange(len(ops)) % 5]
    return hits, ops


def case_random(NP, last_barcode, n=20000, seed=31):
    """B: random hit states on every record, barcode indices from {0, 1, the panel's last, 8 189}."""
    rng = np.random.default_rng(seed)
    hits, ops = blank_reads(NP, n)
    shape = hits.shape
    hits["pdist"] = np.where(rng.random(shape) < 0.3, rng.integers(0, 3, shape), -1)
    hits["bbest"] = np.where(rng.random(shape) < 0.55, rng.integers(0, 3, shape), rng.integers(-2, 0, shape))
    hits["first_tied"] = np.where(hits["bbest"] >= 0, np.array([0, 1, last_barcode, 8189])[rng.integers(0, 4, shape)], -1)
    votes = rng.integers(0, 3, n)                                                 # none, one, or a few anywhere
    hits["flags"] = (rng.random(shape) < 0.15) & (votes[:, None] == 2)
    one = np.flatnonzero(votes == 1)
    hits["flags"][one, rng.integers(0, 2 * NP, len(one))] = 1
    ops["rtype"] = np.where(rng.random(n) < 0.04, R_FILTERED, rng.integers(1, 7, n))
    ops["flags"] = np.array(_OP_FLAGS)[rng.integers(0, 5, n)] * (rng.random(n) < 0.15)
    return hits, ops


def case_bypass(NP, pair, pair1, uses, seed):
    """C: 40 one-row keys with the last slot of the workgroup's table (and of a 64-slot global table) for a home, key j
    uses[j] times, shuffled.  -> (hits, ops, the 40 (b1, b2))."""
    b1, b2 = keys_with_home(pair1, LCAP - 1, LCAP - 1, 40)
    order = np.random.default_rng(seed).permutation(np.repeat(np.arange(40), uses))
    return one_row_reads(NP, pair, b1[order], b2[order]) + (list(zip(b1.tolist(), b2.tolist())),)


# uses of key j in C1 (one workgroup), and in C2 over 8 and over 48 workgroups of 256 reads
BYPASS_USES = {"1+j%6": 1 + np.arange(40) % 6, "8x256": 51 + (np.arange(40) < 8),
               "48x256": 300 + np.arange(40) % 13 + 2 * (np.arange(40) < 27)}
assert [int(u.sum()) for u in BYPASS_USES.values()] == [136, 8 * 256, 48 * 256]


def case_full_table(NP, pair, pair1, n_keys, each=5, seed=41):
    """D: n_keys one-row keys whose home in an 8-slot table is its last slot, `each` times each, shuffled."""
    b1, b2 = keys_with_home(pair1, LCAP - 1, LCAP - 1, n_keys)
    order = np.random.default_rng(seed).permutation(np.repeat(np.arange(n_keys), each))
    return one_row_reads(NP, pair, b1[order], b2[order])


def case_stride(hits_b, ops_b, rows_b, G, seed=51):
    """E: 2 G 256 + 77 reads drawn from 500 templates of case B (rows_b = their rows_per_read): every template also past the
    grid's first step, the 77 reads of the last, partial step on 77 different templates that give rows.
    -> (hits, ops, template of every read, the 500 templates as indices into case B)."""
    rng = np.random.default_rng(seed)
    pool = rng.choice(len(ops_b), 500, replace=False)
    n, step = 2 * G * THREADS + 77, G * THREADS
    assert step >= 500
    use = rng.integers(0, 500, n)
    use[step:step + 500] = rng.permutation(500)
    use[-77:] = rng.permutation([t for t in range(500) if rows_b[pool[t]]])[:77]
    return hits_b[pool[use]], ops_b[pool[use]], use, pool


def case_fallback(n=3000, seed=61):
    """F: reads of case A's kind, about a quarter of the unfiltered ones with SMX_OPF_TRIM_EMPTY."""
    rng = np.random.default_rng(seed)
    hits, ops = case_truth_table()
    at = rng.choice(len(ops), n, replace=False)
    hits, ops = hits[at].copy(), ops[at].copy()
    ops["flags"] = np.where(rng.random(n) < 0.27, OPF_TRIM_EMPTY, 0) | np.where(rng.random(n) < 0.5, OPF_REVERSE, 0)
    return hits, ops


def case_field_edges(NP, pairs):
    """G: on every pair and with every rtype 1..6, one-row reads with barcode fields (8190, 8190), (8190, 0), (0, 8190)."""
    parts = [one_row_reads(NP, pair, [8190, 8190, 0], [8190, 0, 8190], rtype) for pair in pairs for rtype in range(1, 7)]
    return np.concatenate([h for h, _o in parts]), np.concatenate([o for _h, o in parts])


def reference_of_templates(rows_b, pool, use):
    """E's expected (table, fallback list): every template's rows once, times its number of uses."""
    import collections
    table, times = collections.Counter(), np.bincount(use, minlength=len(pool))
    for t, src in enumerate(pool):
        for key in rows_b[src] or []:
            table[key] += int(times[t])
    return table, [i for i, t in enumerate(use.tolist()) if rows_b[pool[t]] is None]


def fields_of(key):
    """(ori, pair1, p1, p2, b1, b2, class, first) of a key, by the layout of include/smx.h."""
    return (key & 3, key >> 2 & 4095, key >> 14 & 1, key >> 15 & 1, key >> 16 & 8191, key >> 29 & 8191, key >> 42 & 7, key >> 45 & 1)


def assert_truth_table_coverage(table, fallback, ops, preorient):
    """What case A must contain for the comparison to mean something, asserted on the reference's own output."""
    fields = [fields_of(key) for key in table]
    assert all(key >> 46 == 0 for key in table)
    assert {f[0] for f in fields} == ({0, 1, 2} if preorient else {0})
    assert {f[6] for f in fields if f[1]} == set(range(6)) and {f[7] for f in fields if f[1]} == {0, 1}
    assert {_SCORE[f[2] + f[3], (f[4] > 0) + (f[5] > 0)] for f in fields if f[1]} == {1, 2, 3, 4, 5}
    assert {(f[4], f[5]) for f in fields if f[1]} >= {(0, 0), (4, 7), (5, 6), (4, 0), (0, 7), (5, 0), (0, 6)}
    filtered, flagged = ops["rtype"] == R_FILTERED, (ops["flags"] & OPF_TRIM_EMPTY) != 0
    assert (filtered & flagged).sum() >= 1000
    assert fallback == np.flatnonzero(flagged & ~filtered).tolist()       # a filtered read is counted, never listed
    none = sum(count for key, count in table.items() if key >> 2 == FIRST >> 2)
    assert none >= int(filtered.sum()) and sum(count for key, count in table.items() if key & FIRST) == len(ops) - len(fallback)


def assert_field_edges(table, n_pairs):
    """Case G: three keys per (pair, class of rtype 1..6), each field decoded by the layout."""
    want = {}
    for pair1 in range(1, n_pairs + 1):
        for cls, times in ((CLASS_FULL, 1), (CLASS_PARTIAL_FWD, 1), (CLASS_PARTIAL_REV, 1), (CLASS_MULTIPLE, 1), (CLASS_UNKNOWN, 2)):
            for b1, b2 in ((8190, 8190), (8190, 0), (0, 8190)):
                want[1, pair1, 1, 1, b1, b2, cls, 1] = times          # UNKNOWN and DEREP_FULL share a class
    assert {fields_of(key): count for key, count in table.items()} == want and len(table) == len(want)
    assert max(fields_of(key)[1] for key in table) == n_pairs
