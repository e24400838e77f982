"""The plain-Python twin of the bimera call and rule (include/smx.h smx_prefix_reach*, specimux_amd/bimera.py), for the
tests: reach by the O(nm) DP of the definition, the keys by a full sort, the verdict from the full matrix of every eligible
parent (not from the two best), and the synthetic plate the tool's tests run on.  Nothing here shares code with the
library's furthest-reaching diagonals or with the tool's top-two rule."""
import json
import random
from typing import Dict, List, Sequence, Tuple

import numpy as np

from specimux_amd import bimera

_MEMO: Dict[Tuple[bytes, bytes], List[int]] = {}


def reach_reference(q: bytes, r: bytes, E: int) -> List[int]:
    """reach(q, r, e) for e = 0..E: D(i, j) = edit distance of q[0:i] and r[0:j] (D(i, 0) = i, D(0, j) = j, exact byte
    equality); reach(e) = the largest i whose row minimum is <= e.  One numpy row per i: the horizontal dependency
    D(i, j) <= D(i, j - 1) + 1 is a running minimum of D(i, j) - j."""
    full = _MEMO.get((q, r))
    if full is None:
        n, m = len(q), len(r)
        ra = np.frombuffer(r, dtype=np.uint8)
        idx = np.arange(m + 1, dtype=np.int64)
        row = idx.copy()
        row_min = [0]
        for i in range(1, n + 1):
            new = np.empty(m + 1, dtype=np.int64)
            new[0] = i
            new[1:] = np.minimum(row[:-1] + (ra != q[i - 1]), row[1:] + 1)
            row = np.minimum.accumulate(new - idx) + idx
            row_min.append(int(row.min()))
        full = [max(i for i in range(n + 1) if row_min[i] <= e) for e in range(bimera.MAX_E + 1)]
        _MEMO[(q, r)] = full
    return full[:E + 1]


def eligible(q: int, t: int, weights: Sequence[int], needs: Sequence[int]) -> bool:
    return t != q and weights[t] >= needs[q]


def matrix_reference(seqs, weights, needs, jobs, E, kernel_ms=None) -> List[np.ndarray]:
    """smx_prefix_reach_matrix: per job [nq, nt, 2, E + 1], 2^32 - 1 where the target is not eligible."""
    out = []
    for q0, nq, t0, nt in jobs:
        m = np.full((nq, nt, 2, E + 1), bimera.NOT_ELIGIBLE, dtype=np.uint32)
        for q in range(q0, q0 + nq):
            for t in range(t0, t0 + nt):
                if eligible(q, t, weights, needs):
                    m[q - q0, t - t0, 0] = reach_reference(seqs[q], seqs[t], E)
                    m[q - q0, t - t0, 1] = reach_reference(seqs[q][::-1], seqs[t][::-1], E)
        out.append(m)
    return out


def keys_reference(seqs, weights, needs, jobs, E, kernel_ms=None) -> np.ndarray:
    """smx_prefix_reach by a full sort of every eligible target's key; the signature of bimera.reach."""
    rows = []
    for (q0, nq, t0, nt), m in zip(jobs, matrix_reference(seqs, weights, needs, jobs, E)):
        for q in range(nq):
            for side in range(2):
                for e in range(E + 1):
                    offers = sorted(bimera.pack_key(int(m[q, t, side, e]), t0 + t) for t in range(nt)
                                    if m[q, t, side, e] != bimera.NOT_ELIGIBLE)
                    rows.append((offers + [bimera.NONE] * bimera.SLOTS)[:bimera.SLOTS])
    return np.array(rows, dtype=np.uint64).reshape(-1)


def classify_reference(n: int, parents: Dict[int, Tuple[List[int], List[int]]], E: int, max_edits: int, min_gain: int):
    """The rule over the full matrix: parents[t] = (left reach per e, right reach per e) of EVERY eligible parent t.
    Returns (status, d1, d2, left, right, el, er, break_lo, break_hi), None where there is none."""
    if not parents:
        return ("no-parents", E + 1, E + 1, None, None, None, None, None, None)
    d1 = min([e for e in range(E + 1) if any(lr[0][e] == n for lr in parents.values())], default=E + 1)
    found = []
    for el in range(E + 1):
        for er in range(E + 1 - el):
            for a, (la, _) in parents.items():
                for b, (_, rb) in parents.items():
                    if a != b and la[el] + rb[er] >= n:
                        # fewest edits, then the smaller el, then the furthest-reaching A (lower index at equal reach),
                        # then the furthest-reaching B
                        found.append((el + er, el, -la[el], a, -rb[er], b, er))
    if not found:
        return ("ok", d1, E + 1, None, None, None, None, None, None)
    d2, el, nla, a, nrb, b, er = min(found)
    status = "chimera" if d2 <= max_edits and d1 - d2 >= min_gain else "ok"
    return (status, d1, d2, a, b, el, er, n + nrb, -nla)


def verdicts_reference(called, parents, scope, max_edits, min_gain, min_parent_ratio):
    """bimera.bimera by the full matrix, sequence by sequence."""
    E = max_edits + min_gain
    ratio = int(round(min_parent_ratio * 1000))
    out = []
    for qi, q in enumerate(called):
        need = bimera.need_of(q.size, ratio)
        full = {}
        for ti, t in enumerate(called):
            if ti != qi and t.size >= need and (scope == "plate" or t.specimen == q.specimen):
                full[ti] = t.seq
        for pi, p in enumerate(parents):
            full[len(called) + pi] = p.seq
        qs = q.seq.encode("latin-1")
        table = {t: (reach_reference(qs, s.encode("latin-1"), E), reach_reference(qs[::-1], s.encode("latin-1")[::-1], E))
                 for t, s in full.items()}
        out.append(classify_reference(len(qs), table, E, max_edits, min_gain))
    return out


def verdict_tuple(v: bimera.Verdict):
    return (v.status, v.d1, v.d2, v.left, v.right, v.el, v.er, v.lo, v.hi)


# ------------------------------------------------------------------------------------------------ the synthetic plate
LENGTH = 160
MAX_EDITS, MIN_GAIN = 2, 3


def _substitute(rng, s: str, positions) -> str:
    out = list(s)
    for p in positions:
        out[p] = rng.choice([c for c in "ACGT" if c != out[p]])
    return "".join(out)


def _edit(rng, s: str, k: int) -> str:
    """k edits (substitution, insertion or deletion) at distinct positions at least 12 from both ends."""
    out = list(s)
    for p in sorted(rng.sample(range(12, len(s) - 12), k), reverse=True):
        kind = rng.randrange(3)
        if kind == 0:
            out[p] = rng.choice([c for c in "ACGT" if c != out[p]])
        elif kind == 1:
            out.insert(p, rng.choice("ACGT"))
        else:
            del out[p]
    return "".join(out)


def _differences(a: str, b: str, lo: int, hi: int) -> int:
    return sum(1 for i in range(lo, hi) if a[i] != b[i])


class Plate:
    """Six wells of two species each (substitution-only divergence from one ancestor, so a breakpoint is exact), four
    haplotypes 1-3 edits from a well's major species, eight chimeras -- six of the two species of their own well, two
    (the last two wells') with the right parent in another well; four of the eight carry 1 or 2 further edits.  Sizes:
    major species 200, minor 80, haplotypes 40, chimeras 10.  truth[name] = (kind, left parent, right parent, breakpoint
    in the record's own coordinates, both parents in the record's well)."""

    def __init__(self, seed: int = 3):
        rng = random.Random(seed)
        ancestor = "".join(rng.choice("ACGT") for _ in range(LENGTH))
        species = [_substitute(rng, ancestor, rng.sample(range(LENGTH), LENGTH // 7)) for _ in range(12)]
        self.called: List[bimera.Called] = []
        self.truth: Dict[str, Tuple] = {}
        counter: Dict[str, int] = {}

        def add(well: int, kind: str, size: int, seq: str, left=None, right=None, bp=None, local=True):
            spec = f"W{well:02d}"
            counter[spec] = counter.get(spec, 0) + 1
            name = f"{spec}_c{counter[spec]}"
            self.called.append(bimera.Called(name, spec, size, f"{name} size={size}", seq))
            self.truth[name] = (kind, left, right, bp, local)
            return name

        names = {}
        for w in range(6):
            names[2 * w] = add(w, "species", 200, species[2 * w])
            names[2 * w + 1] = add(w, "species", 80, species[2 * w + 1])
        for w in (2, 3, 4, 5):
            add(w, "haplotype", 40, _edit(rng, species[2 * w], 1 + w % 3))
        # (well, left species, right species): both orders in wells 0 and 1; the last two take their right parent from well 0
        plan = [(0, 0, 1), (0, 1, 0), (1, 2, 3), (1, 3, 2), (2, 4, 5), (3, 6, 7), (4, 8, 0), (5, 10, 1)]
        need = MAX_EDITS + MIN_GAIN
        for i, (w, a, b) in enumerate(plan):
            ok = [bp for bp in range(40, LENGTH - 39)
                  if min(_differences(species[a], species[b], 0, bp), _differences(species[a], species[b], bp, LENGTH)) >= need]
            bp = rng.choice(ok)
            left, right = species[a][:bp], species[b][bp:]
            if i % 2:                              # half of them: one or two further edits, on either side
                k = 1 + (i // 2) % 2
                on_left = rng.randrange(k + 1)
                left, right = _edit(rng, left, on_left), _edit(rng, right, k - on_left)
            add(w, "chimera", 10, left + right, names[a], names[b], len(left), local=(b // 2 == w))

    def by_specimen(self) -> List[bimera.Called]:
        """The records in the order of consensus_json: specimen after specimen."""
        return sorted(self.called, key=lambda c: c.specimen)       # stable: file order within a specimen

    def consensus_json(self) -> str:
        specimens: Dict[str, List] = {}
        for c in self.called:
            specimens.setdefault(c.specimen, []).append({"name": c.name, "size": c.size, "consensus": c.seq})
        return json.dumps({"specimens": [{"specimen": f"/run/full/{s}.fastq", "clusters": cl} for s, cl in specimens.items()]})
