"""The Python binding of libsmx's one-shot calls (include/smx.h, smx_calls.cpp): the one place that knows their argument
lists.  Five helpers marshal what the calls share -- offsets, limits, job arrays, the trailing kernel_ms argument and the
walk over a flat output -- and one function per entry point allocates that call's outputs (with a sentinel where the
library promises to write every entry), makes the call and returns the outputs cut job after job.  The tools wrap these
in their own types; tests and benches that bring their own buffers call `invoke` directly.

libsmx.so is loaded at the first call, not at import."""
import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

KEY_SENTINEL = 0x5A5A5A5A5A5A5A5A          # never a key the library leaves: it writes every entry
WORD_SENTINEL = 0x5A5A5A5A
ROW_SENTINEL = 0x5A                        # never a byte smx_msa leaves where it promises a row
DIST_SENTINEL = -7                         # never a distance: those are >= -1
ALWAYS = 2**32 - 1                         # the largest weight / need smx_prefix_reach takes
REACH_SLOTS = 2                            # its keys per (query, side, e)


# ------------------------------------------------------------------------------------------------ the helpers
def offsets(seqs: Sequence, dtype=np.uint64) -> np.ndarray:
    """The n + 1 prefix of the lengths of `seqs`: [0] for an empty list."""
    off = np.zeros(len(seqs) + 1, dtype=dtype)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=dtype)
    return off


def limits(ks: Sequence[int]) -> np.ndarray:
    """The limits k as int32."""
    # a negative k means "no limit"; a limit that does not fit 32 bits is no limit either (d <= len(full) always)
    return np.array([min(k, 2**31 - 1) if k >= 0 else -1 for k in ks], dtype=np.int32)


def job_array(jobs: Sequence[tuple], dtype) -> np.ndarray:
    """The jobs (tuples in the order of the record's fields) as a structured array; [] gives a valid array of none."""
    return np.array(list(jobs), dtype=dtype) if len(jobs) else np.zeros(0, dtype=dtype)


def split(flat: np.ndarray, shapes: Sequence) -> List[np.ndarray]:
    """The views of a flat output, one per shape, one after the other."""
    out, at = [], 0
    for shape in shapes:
        n = int(np.prod(shape))
        out.append(flat[at:at + n].reshape(shape))
        at += n
    return out


def invoke(name: str, *args, kernel_ms: Optional[list] = None, check: bool = True) -> int:
    """Call libsmx's `name` with `args` and the float *kernel_ms every one-shot call ends with; the device time is
    appended to `kernel_ms` when that is a list.  Raises SmxError for a nonzero status, or returns it with check=False."""
    ms = C.c_float(0.0)
    status = getattr(_lib.load(), name)(*args, C.byref(ms))
    if check:
        _lib.check(status)
    if kernel_ms is not None:
        kernel_ms.append(ms.value)
    return status


def _filled(n: int, value, dtype) -> np.ndarray:
    """An output of n entries (one at least, so that its pointer is never null) that hold `value`."""
    return np.full(max(n, 1), value, dtype=dtype)


# ------------------------------------------------------------------------------------------------ specimine
def _mine(name, queries, ks, targets, jobs, out, kernel_ms):
    return invoke(name, b"".join(queries), _lib.ptr(offsets(queries)), len(queries), _lib.ptr(limits(ks)), b"".join(targets),
                  _lib.ptr(offsets(targets)), len(targets), _lib.ptr(jobs), len(jobs), _lib.ptr(out), kernel_ms=kernel_ms)


def mine_best_identity(queries: Sequence[bytes], ks: Sequence[int], targets: Sequence[bytes], jobs: Sequence[tuple],
                       kernel_ms: Optional[list] = None) -> np.ndarray:
    """One smx_mine_best_identity call: the full reads (queries) with their limits k (max_distance), the partial reads
    (targets) and the device jobs (q0, nq, t0, nt, min_identity).  Returns the best identity of every job's targets,
    job after job."""
    jarr = np.array(jobs, dtype=_lib.MINE_JOB_DTYPE)
    best = np.zeros(max(int(jarr["nt"].sum()), 1), dtype=np.float64)
    _mine("smx_mine_best_identity", queries, ks, targets, jarr, best, kernel_ms)
    return best


def mine_distances(queries: Sequence[bytes], ks: Sequence[int], targets: Sequence[bytes], jobs: Sequence[tuple],
                   kernel_ms: Optional[list] = None) -> List[np.ndarray]:
    """One smx_mine_distances call: per job its nq x nt distances (-1 above the limit).  For tests and inspection."""
    jarr = job_array(jobs, _lib.MINE_JOB_DTYPE)
    shapes = [(j[1], j[3]) for j in jobs]
    dist = _filled(sum(nq * nt for nq, nt in shapes), DIST_SENTINEL, np.int32)
    _mine("smx_mine_distances", queries, ks, targets, jarr, dist, kernel_ms)
    return split(dist, shapes)


# ------------------------------------------------------------------------------------------------ clusters
def _pairs(name, reads, ks, jobs, out, kernel_ms):
    return invoke(name, b"".join(reads), _lib.ptr(offsets(reads)), len(reads), _lib.ptr(limits(ks)),
                  _lib.ptr(job_array(jobs, _lib.PAIRS_JOB_DTYPE)), len(jobs), _lib.ptr(out), kernel_ms=kernel_ms)


def pairs_neighbours(reads: Sequence[bytes], ks: Sequence[int], jobs: Sequence[Tuple[int, int]],
                     kernel_ms: Optional[list] = None) -> List[np.ndarray]:
    """One smx_pairs_neighbours call: per job (r0, n) its symmetric adjacency bit matrix, n rows x ceil(n / 32) uint32
    words: bit j of row i is set iff i != j and the NW distance of reads i and j is <= max(k[i], k[j])."""
    shapes = [(n, (n + 31) // 32) for _, n in jobs]
    adj = np.zeros(max(sum(n * w for n, w in shapes), 1), dtype=np.uint32)
    _pairs("smx_pairs_neighbours", reads, ks, jobs, adj, kernel_ms)
    return split(adj, shapes)


def pairs_distances(reads: Sequence[bytes], ks: Sequence[int], jobs: Sequence[Tuple[int, int]],
                    kernel_ms: Optional[list] = None) -> List[np.ndarray]:
    """One smx_pairs_distances call: per job its packed upper triangle, row-major over i < j (n (n - 1) / 2 int32, -1
    above the limit).  For tests and inspection."""
    shapes = [n * (n - 1) // 2 for _, n in jobs]
    dist = _filled(sum(shapes), DIST_SENTINEL, np.int32)
    _pairs("smx_pairs_distances", reads, ks, jobs, dist, kernel_ms)
    return split(dist, shapes)


# ------------------------------------------------------------------------------------------------ consensus and its kin
def _cons(name, reads, ks, jobs, *rest, kernel_ms):
    return invoke(name, b"".join(reads), _lib.ptr(offsets(reads)), len(reads), _lib.ptr(limits(ks)),
                  _lib.ptr(job_array(jobs, _lib.CONS_JOB_DTYPE)), len(jobs), *rest, kernel_ms=kernel_ms)


def _vote_outputs(reads, jobs):
    """The shapes of the jobs' vote tables, and the zeroed outputs every vote call fills: the tables and aligned."""
    shapes = [(len(reads[d]) + 1, _lib.CONS_VOTE_WORDS) for d, _, _ in jobs]
    table = np.zeros(max(sum(m for m, _ in shapes) * _lib.CONS_VOTE_WORDS, 1), dtype=np.uint32)
    return shapes, table, np.zeros(max(len(jobs), 1), dtype=np.uint32)


def cons_votes(reads: Sequence[bytes], ks: Sequence[int], jobs: Sequence[Tuple[int, int, int]],
               kernel_ms: Optional[list] = None) -> Tuple[List[np.ndarray], List[int]]:
    """One smx_cons_votes call: per job the (len(draft) + 1) x 26 vote table of its members [r0, r0 + n) aligned to its
    draft, and the number of members that aligned within their limit."""
    shapes, table, aligned = _vote_outputs(reads, jobs)
    _cons("smx_cons_votes", reads, ks, jobs, _lib.ptr(table), _lib.ptr(aligned), kernel_ms=kernel_ms)
    return split(table, shapes), [int(a) for a in aligned[:len(jobs)]]


def cons_pileup(reads: Sequence[bytes], ks: Sequence[int], jobs: Sequence[Tuple[int, int, int]],
                kernel_ms: Optional[list] = None) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """One smx_cons_pileup call: per job its n x (len(draft) + 1) pileup rows and its n distances (-1 above the limit,
    and then a row of 0xFFFFFFFF).  For tests and inspection."""
    shapes = [(n, len(reads[d]) + 1) for d, _, n in jobs]
    rows = _filled(sum(n * m for n, m in shapes), WORD_SENTINEL, np.uint32)
    dist = _filled(sum(n for n, _ in shapes), DIST_SENTINEL, np.int32)
    _cons("smx_cons_pileup", reads, ks, jobs, _lib.ptr(rows), _lib.ptr(dist), kernel_ms=kernel_ms)
    return split(rows, shapes), split(dist, [n for n, _ in shapes])


def cons_phase(reads: Sequence[bytes], ks: Sequence[int], jobs: Sequence[Tuple[int, int, int]], min_permille: int,
               min_reads: int, max_sites: int, kernel_ms: Optional[list] = None):
    """One smx_cons_phase call: per job what cons_votes returns for it (table, aligned), its kept sites (records of
    CONS_SITE_DTYPE), the number of sites that qualified, its allele planes [max_sites, 2, ceil(n / 64)] and its link
    table [max_sites, max_sites, 4]."""
    nj, slots = len(jobs), max_sites
    shapes, table, aligned = _vote_outputs(reads, jobs)
    pshapes = [(slots, 2, (n + 63) // 64) for _, _, n in jobs]
    sites = np.zeros(max(nj * slots, 1), dtype=_lib.CONS_SITE_DTYPE)
    n_sites = np.zeros(max(nj, 1), dtype=np.uint32)
    n_qualified = np.zeros(max(nj, 1), dtype=np.uint32)
    planes = np.zeros(max(sum(pw for _, _, pw in pshapes) * 2 * slots, 1), dtype=np.uint64)
    link = np.zeros(max(nj * slots * slots * 4, 1), dtype=np.uint32)
    _cons("smx_cons_phase", reads, ks, jobs, min_permille, min_reads, max_sites, _lib.ptr(table), _lib.ptr(aligned),
          _lib.ptr(sites), _lib.ptr(n_sites), _lib.ptr(n_qualified), _lib.ptr(planes), _lib.ptr(link), kernel_ms=kernel_ms)
    kept = [sites[j * slots:j * slots + int(n_sites[j])] for j in range(nj)]
    return list(zip(split(table, shapes), [int(a) for a in aligned[:nj]], kept, [int(q) for q in n_qualified[:nj]],
                    split(planes, pshapes), split(link, [(slots, slots, 4)] * nj)))


def cons_resample(reads: Sequence[bytes], ks: Sequence[int], jobs: Sequence[Tuple[int, int, int]], masks: np.ndarray,
                  kernel_ms: Optional[list] = None):
    """One smx_cons_resample call.  masks: n_levels x (the sum of the jobs' n) uint64, the jobs' members in job order.
    Per job what cons_votes returns for it (table, aligned), agree [n_levels, len(draft) + 1] uint64 and the replicates'
    voters [n_levels, 64] uint32."""
    masks = np.ascontiguousarray(masks, dtype=np.uint64)
    n_levels = int(masks.shape[0])
    if masks.ndim != 2 or masks.shape[1] != sum(n for _, _, n in jobs):
        raise ValueError("masks must be n_levels x the number of members")
    nj = len(jobs)
    shapes, table, aligned = _vote_outputs(reads, jobs)
    agree = np.zeros(max(sum(m for m, _ in shapes) * n_levels, 1), dtype=np.uint64)
    sub = np.zeros(max(nj * n_levels * _lib.CONS_REPLICATES, 1), dtype=np.uint32)
    _cons("smx_cons_resample", reads, ks, jobs, _lib.ptr(masks) if masks.size else None, n_levels, _lib.ptr(table),
          _lib.ptr(aligned), _lib.ptr(agree), _lib.ptr(sub), kernel_ms=kernel_ms)
    return list(zip(split(table, shapes), [int(a) for a in aligned[:nj]], split(agree, [(n_levels, m) for m, _ in shapes]),
                    split(sub, [(n_levels, _lib.CONS_REPLICATES)] * nj)))


def cons_profile(reads: Sequence[bytes], quals: Sequence[bytes], ks: Sequence[int], jobs: Sequence[Tuple[int, int, int]],
                 kernel_ms: Optional[list] = None):
    """One smx_cons_profile call.  quals: per read its FASTQ quality bytes, as long as the read (a draft's are never read).
    Per job what cons_votes returns for it (table, aligned), its members' counts [n, 8] uint32 (match, sub, del, other,
    ins_events, ins_bases, clipped, 0) and its SMX_PROFILE_JOB_WORDS table words (q[64][3], subst[4][5], ins[6], hp[8][7])."""
    if len(quals) != len(reads) or any(len(q) != len(r) for q, r in zip(quals, reads)):
        raise ValueError("quals must hold one string per read, of the read's length")
    nj = len(jobs)
    shapes, table, aligned = _vote_outputs(reads, jobs)
    members = _filled(sum(n for _, _, n in jobs) * _lib.PROFILE_MEMBER_WORDS, WORD_SENTINEL, np.uint32)
    tables = _filled(nj * _lib.PROFILE_JOB_WORDS, WORD_SENTINEL, np.uint32)
    _cons("smx_cons_profile", reads, ks, jobs, b"".join(quals), _lib.ptr(table), _lib.ptr(aligned), _lib.ptr(members),
          _lib.ptr(tables), kernel_ms=kernel_ms)
    return list(zip(split(table, shapes), [int(a) for a in aligned[:nj]],
                    split(members, [(n, _lib.PROFILE_MEMBER_WORDS) for _, _, n in jobs]),
                    split(tables, [(_lib.PROFILE_JOB_WORDS,)] * nj)))


# ------------------------------------------------------------------------------------------------ crosstalk
def _nearest(name, seqs, ks, groups, jobs, *outs, kernel_ms):
    return invoke(name, b"".join(seqs), _lib.ptr(offsets(seqs)), len(seqs), _lib.ptr(limits(ks)),
                  _lib.ptr(np.array(groups, dtype=np.uint32)), _lib.ptr(job_array(jobs, _lib.NEAREST_JOB_DTYPE)), len(jobs),
                  *(_lib.ptr(o) for o in outs), kernel_ms=kernel_ms)


def nearest(seqs: Sequence[bytes], ks: Sequence[int], groups: Sequence[int], jobs: Sequence[Tuple[int, int, int, int]],
            kernel_ms: Optional[list] = None) -> Tuple[np.ndarray, np.ndarray]:
    """One smx_nearest call: job after job, per read the key ((d << 32) | ref, 2^64 - 1: none) of the nearest ref of the
    read's own group and of the nearest ref of any other group."""
    n = sum(j[3] for j in jobs)
    own, other = _filled(n, KEY_SENTINEL, np.uint64), _filled(n, KEY_SENTINEL, np.uint64)
    _nearest("smx_nearest", seqs, ks, groups, jobs, own, other, kernel_ms=kernel_ms)
    return own[:n], other[:n]


def nearest_distances(seqs: Sequence[bytes], ks: Sequence[int], groups: Sequence[int],
                      jobs: Sequence[Tuple[int, int, int, int]], kernel_ms: Optional[list] = None) -> List[np.ndarray]:
    """One smx_nearest_distances call: per job its nq x nt distances (-1 above the limit).  For tests and inspection."""
    shapes = [(nq, nt) for _, nq, _, nt in jobs]
    dist = _filled(sum(nq * nt for nq, nt in shapes), DIST_SENTINEL, np.int32)
    _nearest("smx_nearest_distances", seqs, ks, groups, jobs, dist, kernel_ms=kernel_ms)
    return split(dist, shapes)


# ------------------------------------------------------------------------------------------------ identify
def _hits(name, seqs, ks, jobs, K, min_cov_permille, out, kernel_ms):
    return invoke(name, b"".join(seqs), _lib.ptr(offsets(seqs)), len(seqs), _lib.ptr(limits(ks)),
                  _lib.ptr(job_array(jobs, _lib.HITS_JOB_DTYPE)), len(jobs), K, min_cov_permille, _lib.ptr(out),
                  kernel_ms=kernel_ms)


def best_hits(seqs: Sequence[bytes], ks: Sequence[int], jobs: Sequence[Tuple[int, int, int, int]], K: int,
              min_cov_permille: int, kernel_ms: Optional[list] = None) -> np.ndarray:
    """One smx_best_hits call: job after job, per query K keys in ascending order, padded with 2^64 - 1
    (include/smx.h: (d << 20) // len(pattern) in bits 63-43, d in bits 42-24, the target's index in its job below)."""
    n = sum(j[1] for j in jobs) * max(K, 0)
    keys = _filled(n, KEY_SENTINEL, np.uint64)
    _hits("smx_best_hits", seqs, ks, jobs, K, min_cov_permille, keys, kernel_ms)
    return keys[:n]


def best_hits_distances(seqs: Sequence[bytes], ks: Sequence[int], jobs: Sequence[Tuple[int, int, int, int]], K: int,
                        min_cov_permille: int, kernel_ms: Optional[list] = None) -> List[np.ndarray]:
    """One smx_best_hits_distances call: per job its nq x nt distances (-1: above the limit, or excluded by coverage).
    For tests and inspection."""
    shapes = [(nq, nt) for _, nq, _, nt in jobs]
    dist = _filled(sum(nq * nt for nq, nt in shapes), DIST_SENTINEL, np.int32)
    _hits("smx_best_hits_distances", seqs, ks, jobs, K, min_cov_permille, dist, kernel_ms)
    return split(dist, shapes)


# ------------------------------------------------------------------------------------------------ bimera
def _reach(name, seqs, weights, needs, jobs, E, out, kernel_ms):
    warr = np.array([min(int(w), ALWAYS) for w in weights], dtype=np.uint32)
    narr = np.array([min(int(n), ALWAYS) for n in needs], dtype=np.uint32)
    return invoke(name, b"".join(seqs), _lib.ptr(offsets(seqs)), len(seqs), _lib.ptr(warr), _lib.ptr(narr),
                  _lib.ptr(job_array(jobs, _lib.REACH_JOB_DTYPE)), len(jobs), E, _lib.ptr(out), kernel_ms=kernel_ms)


def prefix_reach(seqs: Sequence[bytes], weights: Sequence[int], needs: Sequence[int],
                 jobs: Sequence[Tuple[int, int, int, int]], E: int, kernel_ms: Optional[list] = None) -> np.ndarray:
    """One smx_prefix_reach call: job after job, per query, per side (0 left, 1 right), per e in 0..E, two keys in
    ascending order, padded with 2^64 - 1 (include/smx.h: 0xFFFFFFFF - reach in bits 63-32, the target's index in
    `seqs` below)."""
    n = sum(j[1] for j in jobs) * 2 * (max(E, 0) + 1) * REACH_SLOTS
    keys = _filled(n, KEY_SENTINEL, np.uint64)
    _reach("smx_prefix_reach", seqs, weights, needs, jobs, E, keys, kernel_ms)
    return keys[:n]


def prefix_reach_matrix(seqs: Sequence[bytes], weights: Sequence[int], needs: Sequence[int],
                        jobs: Sequence[Tuple[int, int, int, int]], E: int, kernel_ms: Optional[list] = None) -> List[np.ndarray]:
    """One smx_prefix_reach_matrix call: per job an array [nq, nt, 2, E + 1] (2^32 - 1: the target is not eligible).
    For tests and inspection."""
    shapes = [(nq, nt, 2, max(E, 0) + 1) for _, nq, _, nt in jobs]
    vals = _filled(sum(int(np.prod(s)) for s in shapes), WORD_SENTINEL, np.uint32)
    _reach("smx_prefix_reach_matrix", seqs, weights, needs, jobs, E, vals, kernel_ms)
    return split(vals, shapes)


# ------------------------------------------------------------------------------------------------ tree
def nj(tri, n: int, kernel_ms: Optional[list] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One smx_nj call: the neighbour-joining tree of n tips from their packed upper triangle of distances (n (n - 1) / 2
    int32 >= 0, row-major over i < j, what pairs_distances returns for a job).  Returns the max(n - 3, 0) merge records
    (NJ_MERGE_DTYPE: merge t joins the nodes a and b into the node n + t), the three nodes left (uint32; 0..n-1 for
    n <= 3, the rest 0) and their distances d01, d02, d12 (float64)."""
    n = int(n)
    tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1)
    if n < 0 or tri.size != n * (n - 1) // 2:
        raise ValueError("tri must hold the n (n - 1) / 2 entries of the upper triangle")
    n_merges = max(n - 3, 0)
    merges = _filled(max(n_merges, 1) * (_lib.NJ_MERGE_DTYPE.itemsize // 8), KEY_SENTINEL, np.uint64).view(_lib.NJ_MERGE_DTYPE)
    last = _filled(3, WORD_SENTINEL, np.uint32)
    last_d = _filled(3, KEY_SENTINEL, np.uint64).view(np.float64)
    padded = tri if tri.size else np.zeros(1, dtype=np.int32)      # never a null pointer
    invoke("smx_nj", _lib.ptr(padded), n, _lib.ptr(merges), _lib.ptr(last), _lib.ptr(last_d), kernel_ms=kernel_ms)
    return merges[:n_merges], last, last_d


# ------------------------------------------------------------------------------------------------ msa
def msa(seqs: Sequence[bytes], merges, mismatch: int = 1, gap: int = 1, cap_cols: Optional[int] = None,
        kernel_ms: Optional[list] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One smx_msa call: the n sequences aligned along the guide tree `merges` (n - 1 pairs (a, b): merge t joins the nodes
    a and b into the node n + t; the tips are 0..n-1).  Returns the rows [n, n_cols] uint8 ('-' where a row has a gap),
    the columns of every new node (uint32) and the cost of every merge (uint64).  cap_cols, the room of a row, defaults to
    min(MSA_MAX_COLS, 2 x the longest + 64); if the library reports more columns (SMX_ERR_OVERFLOW) the call is made once
    more with the reported number, and kernel_ms receives both device times."""
    n = len(seqs)
    pairs = [(int(a), int(b)) for a, b in merges]
    if len(pairs) != max(n - 1, 0):
        raise ValueError("merges must hold n - 1 pairs")
    marr = job_array(pairs, _lib.MSA_MERGE_DTYPE) if pairs else np.zeros(1, dtype=_lib.MSA_MERGE_DTYPE)   # never a null pointer
    cap = min(_lib.MSA_MAX_COLS, 2 * max((len(s) for s in seqs), default=0) + 64) if cap_cols is None else int(cap_cols)
    times: list = []
    for attempt in (0, 1):
        rows = _filled(n * cap, ROW_SENTINEL, np.uint8)
        n_cols = _filled(1, WORD_SENTINEL, np.uint32)
        lens = _filled(n - 1, WORD_SENTINEL, np.uint32)
        costs = _filled(n - 1, KEY_SENTINEL, np.uint64)
        status = invoke("smx_msa", b"".join(seqs), _lib.ptr(offsets(seqs)), n, _lib.ptr(marr), int(mismatch), int(gap), cap,
                        _lib.ptr(rows), _lib.ptr(n_cols), _lib.ptr(lens), _lib.ptr(costs), kernel_ms=times, check=False)
        if status == _lib.ERR_OVERFLOW and attempt == 0 and cap < int(n_cols[0]) <= _lib.MSA_MAX_COLS:
            cap = int(n_cols[0])
            continue
        _lib.check(status)
        break
    if kernel_ms is not None:
        kernel_ms.extend(times)
    nc = int(n_cols[0])
    return rows[:n * nc].reshape(n, nc), lens[:max(n - 1, 0)], costs[:max(n - 1, 0)]


# ------------------------------------------------------------------------------------------------ chimera
def _scan(name, head, patterns, k, n, tail, max_hits, kernel_ms):
    """Both inner scans: `head` and `tail` are the arguments before and after (patterns, poff, n_patterns, k)."""
    enc = [p.encode("ascii") for p in patterns]
    kk = np.ascontiguousarray(k, dtype=np.int32)
    q, h = len(enc), int(max_hits)
    nhit, dist, end = np.empty((n, q), dtype=np.uint8), np.empty((n, q, h), dtype=np.int8), np.empty((n, q, h), dtype=np.int32)
    invoke(name, *head, b"".join(enc), _lib.ptr(offsets(enc, np.uint32)), q, _lib.ptr(kk), *tail, _lib.ptr(nhit), _lib.ptr(dist),
           _lib.ptr(end), kernel_ms=kernel_ms)
    return nhit, dist, end


def inner_scan(bases, read_offsets, patterns: Sequence[str], k, margin: int, max_hits: int = 4, budget_bytes: int = 0,
               kernel_ms: Optional[list] = None):
    """smx_inner_scan over reads given as one uint8 array and n + 1 offsets.  Returns (nhit [n, Q] uint8, hit_dist [n, Q, H]
    int8, hit_end [n, Q, H] int32): per read and pattern the number of hits on the internal columns
    margin <= c < len - margin (saturating at 255) and the first max_hits of them in column order (-1 / 0 where unused).
    `kernel_ms` (a list) receives the device time of the call."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    read_offsets = np.ascontiguousarray(read_offsets, dtype=np.uint64)
    n = len(read_offsets) - 1
    return _scan("smx_inner_scan", (), patterns, k, n,
                 (_lib.ptr(bases), _lib.ptr(read_offsets), n, int(margin), int(max_hits), int(budget_bytes)), max_hits, kernel_ms)


def inner_scan_batch(batch, patterns: Sequence[str], k, margin: int, max_hits: int = 4, budget_bytes: int = 0,
                     kernel_ms: Optional[list] = None):
    """The same over a native reader batch (native_io.Batch): libsmx gathers each chunk's sequences from the batch into one
    host staging buffer (one copy per record) and uploads that; no per-record Python work."""
    return _scan("smx_inner_scan_batch", (batch.handle,), patterns, k, len(batch),
                 (int(margin), int(max_hits), int(budget_bytes)), max_hits, kernel_ms)
