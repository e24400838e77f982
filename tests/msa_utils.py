"""The numpy twin of smx_msa and what its tests share, written from the rules of DESIGN.md §23 alone: symbols A C G T / other
/ gap, profiles of six counts, the integer DP of a merge with its tie-break (diagonal, then up, then left), the new
column of an op, rows from the composed maps.  Anti-diagonals are vectorised, so that a 1 025 x 1 025 merge is cheap; the
walk back is a plain loop.  Also: the pairwise cost read off two rows, a brute force over every monotone path of two tiny
profiles, and generators of sequences and guide trees."""
import itertools
from typing import List, Sequence, Tuple

import numpy as np

DIAG, UP, LEFT = 0, 1, 2
GAP = ord("-")
_CODE = np.full(256, 4, dtype=np.int64)
for _k, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _k


def codes_of(seq: bytes) -> np.ndarray:
    return _CODE[np.frombuffer(seq, dtype=np.uint8)]


def tip_profile(seq: bytes) -> np.ndarray:
    """[L, 6] int64, one-hot per base."""
    prof = np.zeros((len(seq), 6), dtype=np.int64)
    prof[np.arange(len(seq)), codes_of(seq)] = 1
    return prof


def merge_costs(pa: np.ndarray, na: int, pb: np.ndarray, nb: int, X: int, G: int):
    """ga [La], gb [Lb], s [La, Lb] as Python-exact int64 (the bound of the issue keeps them below 2^51)."""
    ra, rb = na - pa[:, 5], nb - pb[:, 5]
    ga, gb = G * ra * nb, G * rb * na
    s = X * (np.outer(ra, rb) - pa[:, :5] @ pb[:, :5].T) + G * (np.outer(pa[:, 5], rb) + np.outer(ra, pb[:, 5]))
    return ga, gb, s


def merge_profiles(pa: np.ndarray, na: int, pb: np.ndarray, nb: int, X: int, G: int) -> Tuple[np.ndarray, int]:
    """The ops of the merge in column order (DIAG / UP / LEFT) and its cost D[La][Lb]."""
    La, Lb = len(pa), len(pb)
    ga, gb, s = merge_costs(pa, na, pb, nb, X, G)
    D = np.zeros((La + 1, Lb + 1), dtype=np.int64)
    D[1:, 0] = np.cumsum(ga)
    D[0, 1:] = np.cumsum(gb)
    for d in range(2, La + Lb + 1):
        i = np.arange(max(1, d - Lb), min(La, d - 1) + 1)
        j = d - i
        D[i, j] = np.minimum(np.minimum(D[i - 1, j - 1] + s[i - 1, j - 1], D[i - 1, j] + ga[i - 1]), D[i, j - 1] + gb[j - 1])
    ops, i, j = [], La, Lb
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + s[i - 1, j - 1]:
            ops.append(DIAG)
            i, j = i - 1, j - 1
        elif j == 0 or (i > 0 and D[i, j] == D[i - 1, j] + ga[i - 1]):
            ops.append(UP)
            i -= 1
        else:
            ops.append(LEFT)
            j -= 1
    return np.array(ops[::-1], dtype=np.int64), int(D[La, Lb])


def new_profile(ops: np.ndarray, pa: np.ndarray, na: int, pb: np.ndarray, nb: int) -> np.ndarray:
    prof = np.zeros((len(ops), 6), dtype=np.int64)
    prof[ops != LEFT] += pa
    prof[ops != UP] += pb
    prof[ops == UP, 5] += nb
    prof[ops == LEFT, 5] += na
    return prof


def msa_reference(seqs: Sequence[bytes], merges: Sequence[Tuple[int, int]], X: int = 1, G: int = 1):
    """(rows [n, n_cols] uint8, lens [n - 1] uint32, costs [n - 1] uint64) of the rules, for a valid call."""
    n = len(seqs)
    if n == 0:
        return np.zeros((0, 0), dtype=np.uint8), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64)
    # per node: the tips under it, their rows so far, the profile
    nodes = {i: ([i], np.frombuffer(s, dtype=np.uint8).reshape(1, -1).copy(), tip_profile(s)) for i, s in enumerate(seqs)}
    lens, costs = [], []
    for t, (a, b) in enumerate(merges):
        ta, ma, pa = nodes.pop(int(a))
        tb, mb, pb = nodes.pop(int(b))
        ops, cost = merge_profiles(pa, len(ta), pb, len(tb), X, G)
        m = np.full((len(ta) + len(tb), len(ops)), GAP, dtype=np.uint8)
        m[:len(ta), ops != LEFT] = ma
        m[len(ta):, ops != UP] = mb
        nodes[n + t] = (ta + tb, m, new_profile(ops, pa, len(ta), pb, len(tb)))
        lens.append(len(ops))
        costs.append(cost)
    (tips, m, _), = nodes.values()
    rows = np.empty_like(m)
    rows[np.array(tips)] = m
    return rows, np.array(lens, dtype=np.uint32), np.array(costs, dtype=np.uint64)


def pair_cost_from_rows(x: np.ndarray, y: np.ndarray, X: int, G: int) -> int:
    """The pairwise cost of two rows of one alignment: both gaps 0, one gap G, different symbols X."""
    gx, gy = x == GAP, y == GAP
    differ = ~gx & ~gy & (_CODE[x] != _CODE[y])
    return int(G * np.count_nonzero(gx != gy) + X * np.count_nonzero(differ))


def tips_under(n: int, merges: Sequence[Tuple[int, int]]) -> List[List[int]]:
    under = [[i] for i in range(n)]
    for a, b in merges:
        under.append(under[int(a)] + under[int(b)])
    return under


def brute_force(pa: np.ndarray, na: int, pb: np.ndarray, nb: int, X: int, G: int):
    """Every monotone path of two profiles of <= 4 columns: the smallest cost, among the paths that reach it the one the
    walk back picks -- read from the end, the smallest under diagonal < up < left -- and how many reach it."""
    La, Lb = len(pa), len(pb)
    assert La <= 4 and Lb <= 4
    ga, gb, s = merge_costs(pa, na, pb, nb, X, G)
    best, optimal = None, 0
    for k in range(0, min(La, Lb) + 1):            # k diagonals, La - k ups, Lb - k lefts
        for path in set(itertools.permutations([DIAG] * k + [UP] * (La - k) + [LEFT] * (Lb - k))):
            i = j = cost = 0
            for op in path:
                if op == DIAG:
                    cost += int(s[i, j])
                    i, j = i + 1, j + 1
                elif op == UP:
                    cost += int(ga[i])
                    i += 1
                else:
                    cost += int(gb[j])
                    j += 1
            key = (cost, path[::-1])
            optimal = 1 if best is None or cost < best[0] else optimal + (cost == best[0])
            if best is None or key < best:
                best = key
    return best[0], np.array(best[1][::-1], dtype=np.int64), optimal


# ------------------------------------------------------------------------------------------------ generators
def random_seq(rng, length: int, alphabet: bytes = b"ACGT") -> bytes:
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=length).tolist())


def mutate(rng, seq: bytes, rate: float) -> bytes:
    """Substitutions, insertions and deletions at `rate` per base in all; never empty."""
    out = bytearray()
    for ch in seq:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(int(rng.choice(list(b"ACGT"))))
        elif r < rate:
            out.append(ch)
            out.append(int(rng.choice(list(b"ACGT"))))
        else:
            out.append(ch)
    return bytes(out) or seq[:1]


def family(rng, n: int, length: int, rate: float) -> List[bytes]:
    root = random_seq(rng, length)
    return [mutate(rng, root, rate) for _ in range(n)]


def balanced_tree(n: int) -> List[Tuple[int, int]]:
    merges, nodes = [], list(range(n))
    while len(nodes) > 1:
        nxt = []
        for k in range(0, len(nodes), 2):
            if k + 1 < len(nodes):
                merges.append((nodes[k], nodes[k + 1]))
                nxt.append(n + len(merges) - 1)
            else:
                nxt.append(nodes[k])
        nodes = nxt
    return merges


def ladder_tree(n: int) -> List[Tuple[int, int]]:
    merges, top = [], 0
    for i in range(1, n):
        merges.append((top, i))
        top = n + len(merges) - 1
    return merges


def random_tree(rng, n: int) -> List[Tuple[int, int]]:
    merges, live = [], list(range(n))
    while len(live) > 1:
        a, b = (int(x) for x in rng.choice(len(live), size=2, replace=False))
        merges.append((live[a], live[b]))
        live = [x for k, x in enumerate(live) if k not in (a, b)] + [n + len(merges) - 1]
    return merges
