"""The inner scan's definition in numpy, for the GPU tests of smx_inner_scan and specimux-chimera: a plain last-row DP with
the equality relation of specimux_amd.constants, and the hits it implies."""
import numpy as np

from specimux_amd.constants import IUPAC_EQUIV

LETTERS = "ACGTNRYKMSWBDHV"
# EQ[pattern letter, read byte]: identity on the 15 letters plus the 28 symmetric pairs; any other read byte matches nothing
EQ = np.zeros((256, 256), dtype=bool)
for _c in LETTERS:
    EQ[ord(_c), ord(_c)] = True
for _a, _b in IUPAC_EQUIV:
    EQ[ord(_a), ord(_b)] = EQ[ord(_b), ord(_a)] = True


def last_row(pattern, read):
    """D(c) for every column: row by row, the horizontal dependency resolved by a running minimum of (value - column)."""
    n = len(read)
    t = np.frombuffer(read, dtype=np.uint8)
    idx = np.arange(n + 1, dtype=np.int64)        # position 0 is the fresh column in front of the read: D[i][-1] = i
    prev = np.zeros(n + 1, dtype=np.int64)
    for i, ch in enumerate(pattern.encode(), start=1):
        tmp = np.empty(n + 1, dtype=np.int64)
        tmp[0] = i
        tmp[1:] = np.minimum(prev[:-1] + ~EQ[ch][t], prev[1:] + 1)
        prev = np.minimum.accumulate(tmp - idx) + idx
    return prev[1:]


def expected(patterns, ks, reads, margin, H):
    n, Q = len(reads), len(patterns)
    nhit = np.zeros((n, Q), dtype=np.uint8)
    dist = np.full((n, Q, H), -1, dtype=np.int8)
    end = np.zeros((n, Q, H), dtype=np.int32)
    for r, read in enumerate(reads):
        if len(read) <= 2 * margin:
            continue
        for j, (p, k) in enumerate(zip(patterns, ks)):
            D = last_row(p, read)
            ok = np.zeros(len(read) + 2, dtype=bool)
            ok[1 + margin:1 + len(read) - margin] = D[margin:len(read) - margin] <= k
            starts = np.flatnonzero(ok[1:-1] & ~ok[:-2])
            stops = np.flatnonzero(ok[1:-1] & ~ok[2:])
            nhit[r, j] = min(len(starts), 255)
            for h, (a, b) in enumerate(zip(starts[:H], stops[:H])):
                dist[r, j, h] = D[a:b + 1].min()
                end[r, j, h] = a + int(np.argmin(D[a:b + 1]))
    return nhit, dist, end


def flat(reads):
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads) + b"\0", dtype=np.uint8)[:-1].copy(), off
