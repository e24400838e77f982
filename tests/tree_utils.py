"""What the tree tests share: the twin of smx_nj in numpy float64 (nj_reference), written from DESIGN.md §22 and
include/smx.h, not from the kernel; the same algorithm in exact fractions with the row sums recomputed every iteration
(nj_exact), an independent statement of neighbour joining; a scalar float version that counts its inexact operations;
generators of additive and other matrices; a Newick reader; and a small synthetic plate for the tool."""
import random
from fractions import Fraction

import numpy as np

MERGE = np.dtype([("a", "<u4"), ("b", "<u4"), ("n_active", "<u4"), ("pad", "<u4"), ("d", "<f8"), ("ra", "<f8"), ("rb", "<f8")])


# ------------------------------------------------------------------------------------------------ matrices
def tri_of(D) -> np.ndarray:
    """The packed upper triangle of a square matrix, row-major over i < j."""
    D = np.asarray(D)
    return np.ascontiguousarray(D[np.triu_indices(D.shape[0], 1)], dtype=np.int32)


def full_of(tri, n: int) -> np.ndarray:
    D = np.zeros((n, n), dtype=np.int64)
    D[np.triu_indices(n, 1)] = np.asarray(tri, dtype=np.int64)
    return D + D.T


def random_matrix(rng: random.Random, n: int, lo: int = 1, hi: int = 3000) -> np.ndarray:
    D = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        for j in range(i + 1, n):
            D[i, j] = D[j, i] = rng.randint(lo, hi)
    return D


def random_matrix_np(seed: int, n: int, lo: int = 1, hi: int = 3000) -> np.ndarray:
    """The same kind of matrix for large n."""
    U = np.triu(np.random.default_rng(seed).integers(lo, hi + 1, size=(n, n), dtype=np.int64), 1)
    return U + U.T


def constant_matrix(n: int, value: int) -> np.ndarray:
    return np.full((n, n), value, dtype=np.int64) - value * np.eye(n, dtype=np.int64)


def ladder_matrix(n: int) -> np.ndarray:
    """D[i][j] = 3 max(i, j) + 1 + (i + j) % 2: its recorded values need more than 53 bits."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    D = 3 * np.maximum(i, j) + 1 + (i + j) % 2
    D[np.arange(n), np.arange(n)] = 0
    return D.astype(np.int64)


def additive_matrix(seed: int, n: int):
    """A random binary tree on n >= 3 tips with integer branch lengths 1..50: its tip distances (n x n int64) and its
    branches as {split: length}, a split being the frozenset of the tips on the side without tip 0."""
    rng = random.Random(seed)
    D = np.zeros((n, n), dtype=np.int64)
    everyone = frozenset(range(n))
    clusters = [(np.array([i]), np.zeros(1, dtype=np.int64)) for i in range(n)]     # (tips, root-to-tip distances)
    splits = {}

    def close(tips, length):
        side = frozenset(int(t) for t in tips)
        splits[everyone - side if 0 in side else side] = length

    while len(clusters) > 3:
        a = clusters.pop(rng.randrange(len(clusters)))
        b = clusters.pop(rng.randrange(len(clusters)))
        la, lb = rng.randint(1, 50), rng.randint(1, 50)
        close(a[0], la)
        close(b[0], lb)
        ha, hb = a[1] + la, b[1] + lb
        D[np.ix_(a[0], b[0])] = ha[:, None] + hb[None, :]
        clusters.append((np.concatenate([a[0], b[0]]), np.concatenate([ha, hb])))
    hs = []
    for tips, h in clusters:
        length = rng.randint(1, 50)
        close(tips, length)
        hs.append(h + length)
    for x in range(3):
        for y in range(x + 1, 3):
            D[np.ix_(clusters[x][0], clusters[y][0])] = hs[x][:, None] + hs[y][None, :]
    D = np.maximum(D, D.T)
    return D, splits


# ------------------------------------------------------------------------------------------------ the twin
def nj_reference(D):
    """smx_nj on the host: numpy float64, one rounded operation per numpy operation (elementwise numpy does not fuse).
    D: n x n symmetric integers.  Returns (merges, last, last_d) as calls.nj does."""
    D = np.asarray(D)
    n = D.shape[0]
    merges = np.zeros(max(n - 3, 0), dtype=MERGE)
    last, last_d = np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.float64)
    if n <= 3:
        last[:n] = np.arange(n)
        if n == 2:
            last_d[0] = D[0, 1]
        if n == 3:
            last_d[:] = (D[0, 1], D[0, 2], D[1, 2])
        return merges, last, last_d
    d = D.astype(np.float64)
    r = D.astype(np.int64).sum(axis=1).astype(np.float64)
    node = np.arange(n, dtype=np.uint32)
    lower = np.where(np.tri(n, dtype=bool), np.inf, 0.0)      # +inf on and below the diagonal: only lo < hi competes
    Q = np.empty((n, n), dtype=np.float64)
    na = n
    for t in range(n - 3):
        c = float(na - 2)
        q, dd = Q[:na, :na], d[:na, :na]
        np.multiply(dd, c, out=q)
        np.subtract(q, r[:na, None], out=q)                   # the smaller slot's r first: the row's
        np.subtract(q, r[None, :na], out=q)
        np.add(q, lower[:na, :na], out=q)
        lo, hi = divmod(int(np.argmin(q)), na)                # the first smallest in row-major order: smallest lo, then hi
        dl, ra, rb = d[lo, hi], r[lo], r[hi]
        merges[t] = (node[lo], node[hi], na, 0, dl, ra, rb)
        keep = np.ones(na, dtype=bool)
        keep[[lo, hi]] = False
        a, b = d[lo, :na][keep], d[hi, :na][keep]
        duk = 0.5 * ((a + b) - dl)
        r[:na][keep] = ((r[:na][keep] - a) - b) + duk
        r[lo] = 0.5 * ((ra + rb) - float(na) * dl)
        d[lo, :na][keep] = duk
        d[:na, lo][keep] = duk
        node[lo] = n + t
        if hi != na - 1:
            d[hi, :na] = d[na - 1, :na]
            d[:na, hi] = d[:na, na - 1]
            r[hi], node[hi] = r[na - 1], node[na - 1]
        d[hi, hi] = 0.0
        na -= 1
    last[:] = node[:3]
    last_d[:] = (d[0, 1], d[0, 2], d[1, 2])
    return merges, last, last_d


def nj_scalar(D, exact_check: bool = False):
    """The same in plain Python floats, one operation per statement.  With exact_check every operation is redone in
    fractions: returns (merges, last, last_d, number of operations whose result was rounded)."""
    n = len(D)
    inexact = 0

    def op(f, x, y):
        nonlocal inexact
        z = f(x, y)
        if exact_check and Fraction(z) != f(Fraction(x), Fraction(y)):
            inexact += 1
        return z

    mul, add, sub = (lambda x, y: x * y), (lambda x, y: x + y), (lambda x, y: x - y)
    d = [[float(D[i][j]) for j in range(n)] for i in range(n)]
    r = [float(sum(int(D[i][j]) for j in range(n))) for i in range(n)]
    node = list(range(n))
    merges = np.zeros(max(n - 3, 0), dtype=MERGE)
    na = n
    for t in range(max(n - 3, 0)):
        c = float(na - 2)
        best = None
        for lo in range(na):
            for hi in range(lo + 1, na):
                q = op(sub, op(sub, op(mul, c, d[lo][hi]), r[lo]), r[hi])
                if best is None or q < best[0]:
                    best = (q, lo, hi)
        _, lo, hi = best
        dl, ra, rb = d[lo][hi], r[lo], r[hi]
        merges[t] = (node[lo], node[hi], na, 0, dl, ra, rb)
        for k in range(na):
            if k in (lo, hi):
                continue
            duk = op(mul, 0.5, op(sub, op(add, d[lo][k], d[hi][k]), dl))
            r[k] = op(add, op(sub, op(sub, r[k], d[lo][k]), d[hi][k]), duk)
            d[lo][k] = d[k][lo] = duk
        r[lo] = op(mul, 0.5, op(sub, op(add, ra, rb), op(mul, float(na), dl)))
        node[lo] = n + t
        last = na - 1
        if hi != last:
            for k in range(na):
                d[hi][k] = d[last][k]
            for k in range(na):
                d[k][hi] = d[k][last]
            r[hi], node[hi] = r[last], node[last]
        d[hi][hi] = 0.0
        na -= 1
    lastn, last_d = np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.float64)
    lastn[:min(n, 3)] = node[:min(n, 3)]
    if n == 2:
        last_d[0] = d[0][1]
    if n >= 3:
        last_d[:] = (d[0][1], d[0][2], d[1][2])
    return merges, lastn, last_d, inexact


def nj_exact(D):
    """Neighbour joining in exact fractions, r recomputed as the true row sums every iteration; the tie rule is the
    call's.  Returns (merges as tuples (a, b, n_active, d, ra, rb), last, last_d) with Fractions."""
    n = len(D)
    d = [[Fraction(int(D[i][j])) for j in range(n)] for i in range(n)]
    node = list(range(n))
    merges = []
    na = n
    for t in range(max(n - 3, 0)):
        r = [sum(d[i][:na]) for i in range(na)]
        best = None
        for lo in range(na):
            for hi in range(lo + 1, na):
                q = (na - 2) * d[lo][hi] - r[lo] - r[hi]
                if best is None or q < best[0]:
                    best = (q, lo, hi)
        _, lo, hi = best
        dl = d[lo][hi]
        merges.append((node[lo], node[hi], na, dl, r[lo], r[hi]))
        for k in range(na):
            if k not in (lo, hi):
                d[lo][k] = d[k][lo] = (d[lo][k] + d[hi][k] - dl) / 2
        node[lo] = n + t
        last = na - 1
        if hi != last:
            for k in range(na):
                d[hi][k] = d[last][k]
            for k in range(na):
                d[k][hi] = d[k][last]
            node[hi] = node[last]
        d[hi][hi] = Fraction(0)
        na -= 1
    m = min(n, 3)
    last_d = [Fraction(0)] * 3
    if n == 2:
        last_d[0] = d[0][1]
    if n >= 3:
        last_d = [d[0][1], d[0][2], d[1][2]]
    return merges, node[:m] + [0] * (3 - m), last_d


def same_records(got, want) -> bool:
    """Two (merges, last, last_d) results equal byte for byte: doubles compared as bits."""
    return all(np.asarray(g).dtype == np.asarray(w).dtype and np.asarray(g).shape == np.asarray(w).shape
               and np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ trees
def splits_of_result(n: int, merges, last, last_d):
    """{split: branch length} of a (merges, last, last_d) result, by the host-side formulas of include/smx.h; a split is
    the frozenset of the tips on the side without tip 0."""
    everyone = frozenset(range(n))
    tips = {i: frozenset([i]) for i in range(n)}
    out = {}

    def put(side, length):
        out[everyone - side if 0 in side else side] = length

    for t, m in enumerate(merges):
        a, b, na = int(m["a"]), int(m["b"]), int(m["n_active"])
        d, ra, rb = float(m["d"]), float(m["ra"]), float(m["rb"])
        la = 0.5 * d + (ra - rb) / (2 * (na - 2))
        put(tips[a], la)
        put(tips[b], d - la)
        tips[n + t] = tips[a] | tips[b]
    d01, d02, d12 = (float(x) for x in last_d)
    for x, length in zip(last, (0.5 * (d01 + d02 - d12), 0.5 * (d01 + d12 - d02), 0.5 * (d02 + d12 - d01))):
        put(tips[int(x)], length)
    return out


def read_newick(text: str):
    """{split: length} of a Newick string, a split being the frozenset of the tip labels on the side without the first
    label of the text; the root's own entry is left out."""
    text = text.strip()
    assert text.endswith(";")
    pos = 0
    order, entries = [], []                       # labels in text order; (labels below, length)

    def node():
        nonlocal pos
        below = []
        if text[pos] == "(":
            pos += 1
            while True:
                below += node()
                if text[pos] == ",":
                    pos += 1
                    continue
                assert text[pos] == ")", (pos, text[pos])
                pos += 1
                break
        start = pos
        while text[pos] not in ",():;":
            pos += 1
        label = text[start:pos]
        if not below:
            assert label, "a tip needs a label"
            order.append(label)
            below = [label]
        length = None
        if text[pos] == ":":
            start = pos = pos + 1
            while text[pos] not in ",();":
                pos += 1
            length = float(text[start:pos])
        entries.append((frozenset(below), length))
        return below

    node()
    assert text[pos] == ";" and len(set(order)) == len(order)
    everyone = frozenset(order)
    out = {}
    for below, length in entries[:-1]:            # the last entry is the root
        out[everyone - below if order[0] in below else below] = length
    return out


# ------------------------------------------------------------------------------------------------ the tool's twins
def nw_distance(a: bytes, b: bytes) -> int:
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (ca != cb), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


def edits_twin(seqs, ks, kernel_ms=None) -> np.ndarray:
    """tree.device_edits on the host: the packed triangle of NW distances, -1 above max(k_i, k_j)."""
    out = []
    for i in range(len(seqs)):
        for j in range(i + 1, len(seqs)):
            e = nw_distance(seqs[i], seqs[j])
            out.append(e if e <= max(ks[i], ks[j]) else -1)
    return np.array(out, dtype=np.int32)


def nj_twin(tri, n, kernel_ms=None):
    """calls.nj on the host."""
    return nj_reference(full_of(tri, n))


def synthetic_plate(seed: int = 11, groups: int = 3, per_group: int = 4, length: int = 120):
    """(names, sequences): `groups` unrelated sequences, each with per_group near-identical copies (0..2 substitutions)."""
    rng = random.Random(seed)
    names, seqs = [], []
    for g in range(groups):
        base = [rng.choice("ACGT") for _ in range(length + 3 * g)]
        for i in range(per_group):
            s = list(base)
            for _ in range(i % 3):
                at = rng.randrange(len(s))
                s[at] = rng.choice([c for c in "ACGT" if c != s[at]])
            names.append(f"g{g}_s{i}")
            seqs.append("".join(s))
    return names, seqs


def fasta_text(names, seqs) -> str:
    return "".join(f">{n}\n{s}\n" for n, s in zip(names, seqs))
