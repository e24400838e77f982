"""A plain twin of the barcode survey's two kernels (include/smx.h, "Barcode survey"), independent of flank_shw, flank_take
and flank_of_hit (specimux_amd/csrc/smx_flank_core.h):

  make_key / key_parts      the key layout, written out from the header's table
  assign_reference          best / first / ntied of every key over its primer's candidates in the caller's order.  The
                            distance is edlib's SHW with the candidate as query and the flank as target, straight from
                            oracle.edlib_semantics.align_c, cached by (candidate, flank)
  stats_hash                smx_stats_core.h's hash restated, to steer keys into chosen table slots
  count_reference           brute_force of tests/test_flank_gpu.py restated over numpy arrays (hit records, windows, lens)
"""
import numpy as np

from oracle.edlib_semantics import SHW, align_c

LEN_SHIFT, MATCHED_SHIFT, PRIMER_SHIFT, MAX_W = 52, 57, 58, 26
HITS, PRUNED, SHORT_READ, SHORT_FLANK, AMBIGUOUS, COUNTED = range(6)


def make_key(flank, matched, primer):
    """[0, 52) the flank, 2 bits per base, A C G T = 0 1 2 3, base t at bits [2 t, 2 t + 2); [52, 57) its length;
    57 matched; [58, 64) the primer."""
    assert len(flank) <= MAX_W and 0 <= primer < 64 and matched in (0, 1)
    bits = 0
    for t, ch in enumerate(flank):
        bits |= "ACGT".index(ch) << (2 * t)
    return bits | len(flank) << LEN_SHIFT | matched << MATCHED_SHIFT | primer << PRIMER_SHIFT


def key_parts(key):
    """key -> (flank string, matched, primer)."""
    key = int(key)
    flen = key >> LEN_SHIFT & 31
    return "".join("ACGT"[key >> (2 * t) & 3] for t in range(flen)), key >> MATCHED_SHIFT & 1, key >> PRIMER_SHIFT & 63


_DIST = {}   # (candidate, flank) -> distance: the tests share candidates and flanks


def shw_distance(cand, flank):
    """edlib's SHW distance, candidate as query and flank as target, IUPAC equalities: the suite's oracle, as it is."""
    d = _DIST.get((cand, flank))
    if d is None:
        d = _DIST[(cand, flank)] = align_c(cand, flank, SHW, -1, iupac=True)["editDistance"]
    return d


def assign_reference(keys, candidates, k, stats=None):
    """(best, first, ntied) int32 arrays by the rule of include/smx.h: over the candidates of the key's primer, in the
    caller's order, the least distance <= k, the first caller index that attains it, how many attain it; (-1, -1, 0) when
    none does.  candidates = [(primer, string)].  stats (dict) receives "dists" = {key position: [(caller index, distance)]
    over the primer's candidates}, for the tests to assert on that their fixtures reach the edges they are after."""
    n = len(keys)
    best, first, ntied = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    of_primer = {}
    for c, (p, seq) in enumerate(candidates):                                  # caller's order
        of_primer.setdefault(p, []).append((c, seq))
    done = {}
    for i, key in enumerate(keys):
        flank, _matched, p = key_parts(key)
        if (flank, p) not in done:
            done[(flank, p)] = [(c, shw_distance(seq, flank)) for c, seq in of_primer.get(p, [])]
        dists = done[(flank, p)]
        if stats is not None:
            stats.setdefault("dists", {})[i] = dists
        within = [d for _c, d in dists if d <= k]
        if within:
            best[i] = min(within)
            attain = [c for c, d in dists if d == best[i]]
            first[i], ntied[i] = attain[0], len(attain)
    return best, first, ntied


# ------------------------------------------------------------------------------------------------ the count kernel
def stats_hash(key):
    """smx_stats_core.h stats_hash: xor-shift 29, Fibonacci multiplier, the high 32 bits."""
    key = int(key) & (1 << 64) - 1
    key ^= key >> 29
    key = key * 0x9E3779B97F4A7C15 & (1 << 64) - 1
    return key >> 32


_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b
_CODE = np.full(256, -1, dtype=np.int64)
for _i, _a in enumerate(b"ACGT"):
    _CODE[_a] = _i


def count_reference(S, Lb, k, windows, lens, hits):
    """The definitions of include/smx.h in numpy, one row per (read, primer, end) hit record: returns (table {key: count},
    counters [NP, 6] uint64, categories [n, 2 NP] (0 = no hit), keys [n, 2 NP] uint64 (valid where COUNTED))."""
    n, H = hits.shape
    NP, W = H // 2, Lb + k
    lens = np.asarray(lens, dtype=np.int64)
    L = np.broadcast_to(lens[:, None], (n, H))
    end = np.broadcast_to(np.arange(H)[None, :] & 1, (n, H))
    primer = np.broadcast_to(np.arange(H)[None, :] >> 1, (n, H))
    # the end strings' last S letters: the tail window, and the reverse complement of the head window
    tail = windows[:, S:2 * S]
    head_rc = _COMP[windows[:, :S][:, ::-1]]
    j_end = hits["first_end"].astype(np.int64) - (L - S)
    flen = np.clip(S - 1 - j_end, 0, W)
    cat = np.zeros((n, H), dtype=np.int64)
    is_hit = hits["pdist"] >= 0
    pruned = is_hit & (hits["bbest"] == -2)
    short_read = is_hit & ~pruned & (L < S)
    rest = is_hit & ~pruned & ~short_read
    assert ((j_end >= 0) & (j_end < S))[rest].all()
    short_flank = rest & (flen < Lb - k)
    rest &= ~short_flank
    # the flank's letters: column t of row (i, h) is end_string[j_end + 1 + t], read only where t < flen
    t = np.arange(W)[None, None, :]
    pos = np.clip(j_end[:, :, None] + 1 + t, 0, S - 1)                      # (clipped: records that are no counted hit)
    rows = np.arange(n)[:, None, None]
    letters = np.where(end[:, :, None] == 1, tail[rows, pos], head_rc[rows, pos])
    code = _CODE[letters]
    live = t < flen[:, :, None]
    ambiguous = rest & ((code < 0) & live).any(axis=2)
    counted = rest & ~ambiguous
    bits = (np.where(live & (code >= 0), code, 0).astype(np.uint64) << (2 * np.arange(W, dtype=np.uint64))[None, None, :]).sum(
        axis=2, dtype=np.uint64)
    keys = bits | flen.astype(np.uint64) << np.uint64(LEN_SHIFT) | (hits["bbest"] >= 0).astype(np.uint64) << np.uint64(MATCHED_SHIFT) \
        | primer.astype(np.uint64) << np.uint64(PRIMER_SHIFT)
    for mask, c in ((pruned, PRUNED), (short_read, SHORT_READ), (short_flank, SHORT_FLANK), (ambiguous, AMBIGUOUS), (counted, COUNTED)):
        cat[mask] = c
    counters = np.zeros((NP, 6), dtype=np.uint64)
    for c in range(1, 6):
        counters[:, c] = np.bincount(primer[cat == c], minlength=NP)
    counters[:, HITS] = counters[:, 1:].sum(axis=1)
    uniq, cnt = np.unique(keys[counted], return_counts=True)
    return dict(zip(uniq.tolist(), cnt.tolist())), counters, cat, keys
