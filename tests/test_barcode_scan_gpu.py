"""The demux kernel's bit-sliced barcode scans (smx_barcode_core.h) on the GPU, at the barcode lengths and k where they go
wrong: every padded height (and m <= 3, which runs at 16 rows), k from 0 to 7 with k = m - 1, the k = 3 default-flags
kernels, --trim tails, a partly filled second 32-barcode word, and an m = 17 control on the per-barcode path.

Reads are built explicitly -- primer, barcode with exactly d = 0..k+1 edits at its ends, insert -- plus ties between
two barcodes, N / R inside the barcode, reads cut inside the barcode by the read end, and a slice of synth reads.  Hit
tables (slots and lean) and write operations are compared with the oracle, and the oracle's hit tables must show
that the edges are reached: hits at exactly k, tied hits, and hits with no barcode within k."""
import random

import pytest

from parity_utils import Both, reads_from_set, tmp_panel

pytestmark = pytest.mark.gpu

S = 80


@pytest.fixture(scope="module")
def lib():
    import ctypes as C
    from specimux_amd import _lib
    lib = _lib.load()
    n = C.c_int(0)
    _lib.check(lib.smx_device_init(0, C.byref(n)))
    assert n.value >= 1
    return lib


def _barcodes(rng, n, m, taken):
    """n distinct random barcodes of length m; the second differs from the first in one position (ties)."""
    out = []
    while len(out) < n:
        if len(out) == 1 and m > 0:
            p = rng.randrange(m)
            b = out[0][:p] + rng.choice([c for c in "ACGT" if c != out[0][p]]) + out[0][p + 1:]
        else:
            b = "".join(rng.choice("ACGT") for _ in range(m))
        if b not in taken:
            taken.add(b)
            out.append(b)
    return out


def _panel(tmp_path_factory, name, m, n_fwd, n_rev, seed):
    from specimux_amd import synth
    rng = random.Random(seed)
    taken = set()
    f = _barcodes(rng, n_fwd, m, taken)
    r = [synth.revcomp(b) for b in _barcodes(rng, n_rev, m, taken)]
    pools = [("ITS", "FWD", synth.ITS1F, "ITS4", synth.ITS4)]
    pan = synth.Panel(pools, f, r)
    return pan, tmp_panel(tmp_path_factory, pan, name)


def _edit_ends(rng, b, d):
    """b with exactly d edits (substitution, insertion, deletion), each at its first or last base"""
    s = list(b)
    for _ in range(d):
        front = rng.random() < 0.5
        op = rng.randrange(3) if s else 1
        pos = 0 if front else len(s) - 1
        if op == 0:
            s[pos] = rng.choice([c for c in "ACGT" if c != s[pos]])
        elif op == 1:
            s.insert(0 if front else len(s), rng.choice("ACGT"))
        else:
            del s[pos]
    return "".join(s)


def _reads(pan, k, seed):
    from specimux_amd import synth
    rng = random.Random(seed)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))  # noqa: E731
    ins = rnd(320)
    P1, P2rc = synth.ITS1F, synth.revcomp(synth.ITS4)
    f, r = pan.fwd, pan.rev
    m = len(f[0])
    out = []

    def add(name, b1, b2, lead=None, trail=None, flip=None):
        s = (rnd(rng.randrange(0, 6)) if lead is None else lead) + b1 + P1 + ins + P2rc + synth.revcomp(b2) + \
            (rnd(rng.randrange(0, 6)) if trail is None else trail)
        if flip if flip is not None else rng.random() < 0.5:
            s = synth.revcomp(s)
        out.append((f"{name}_{len(out)}", s, "I" * len(s)))

    # exactly d edits at the barcode's ends, d = 0..k+1, on either barcode
    for d in range(k + 2):
        for _ in range(6):
            b1, b2 = rng.choice(f), rng.choice(r)
            if rng.random() < 0.5:
                add(f"d{d}f", _edit_ends(rng, b1, d), b2)
            else:
                add(f"d{d}r", b1, _edit_ends(rng, b2, d))
    # ties: the position where the first two barcodes of a side differ set to N, or to a third letter
    for side, (x, y) in enumerate(((f[0], f[1]), (r[0], r[1]))):
        p = next(i for i in range(m) if x[i] != y[i])
        third = next(c for c in "ACGT" if c not in (x[p], y[p]))
        for c in ("N", third, "N", third):
            t = x[:p] + c + x[p + 1:]
            add("tie", t, rng.choice(r)) if side == 0 else add("tie", rng.choice(f), t)
    # N and R inside the barcode region
    for c in "NR":
        for _ in range(2):
            b1 = rng.choice(f)
            q = rng.randrange(m)
            add("iupac", b1[:q] + c + b1[q + 1:], rng.choice(r))
    # the read starts / ends inside the barcode (its target is cut by the window end), or right at the primer
    for cut in range(0, m + k + 2):
        b1, b2 = rng.choice(f), rng.choice(r)
        add("cutf", (rnd(k + 2) + b1)[-cut:] if cut else "", b2, lead="", flip=False)
        add("cutr", b1, (b2 + rnd(k + 2))[:cut] if cut else "", trail="", flip=False)
    # reads cut within the search window: short inserts
    for L in (m + len(P1) + 3, m + len(P1) + 20, 70):
        b1 = rng.choice(f)
        out.append((f"short_{len(out)}", (b1 + P1 + ins)[:L], "I" * L))
    if m >= 2:   # (the generator truncates reads inside the barcode: it needs m >= 2)
        rs = synth.make_reads(pan, 40, seed + 1, windows_only=False)
        out += reads_from_set(rs, range(40), S, prefix="syn")
    return out


def _coverage(both, reads, k):
    """(hits at exactly k, tied hits, hits with a primer but no barcode within k) in the oracle's hit tables"""
    from oracle import specimux_oracle as O
    at_k = tied = none = 0
    for rec in reads:
        for v in O.hit_table(both.opar, both.opanel, rec).values():
            if v["pdist"] < 0:
                continue
            d = [x for x, _ in v["barcodes"].values()]
            if not d:
                none += 1
                continue
            best = min(d)
            at_k += best == k
            tied += d.count(best) >= 2
    return at_k, tied, none


GRID = ([(3, m) for m in (4, 5, 8, 9, 12, 13, 14, 16)]
        + [(k, m) for k in (0, 1, 2) for m in (1, 2, 3, 4, 8, 13, 16) if k < m]
        + [(4, m) for m in (5, 13, 16)]
        + [(k, m) for k in (5, 7) for m in (8, 16)])


@pytest.mark.parametrize("k,m", GRID, ids=lambda v: str(v))
def test_barcode_scan_edges(lib, tmp_path_factory, k, m):
    n_fwd, n_rev = (2, 2) if m == 1 else (6, 4)
    pan, (pf, sf) = _panel(tmp_path_factory, f"bs_k{k}_m{m}", m, n_fwd, n_rev, seed=100 * k + m)
    reads = _reads(pan, k, seed=1000 + 100 * k + m)
    base = dict(index_edit_distance=k)
    if m - k < 2:
        base["disable_prefilter"] = True   # the prefilter's minimum length m - k must be >= 2
    flag_sets = [base, dict(base, trim="tails")]
    if k == 0 and "disable_prefilter" not in base:   # the exact-set prefilter drops N reads: k = 0 ties need it off
        flag_sets.append(dict(base, disable_prefilter=True))
    cov = [0, 0, 0]
    for fl in flag_sets:
        both = Both(pf, sf, **fl)
        both.assert_hits_equal(reads, f"k={k} m={m} {fl}")
        both.assert_ops_equal(reads, f"k={k} m={m} {fl}")
        cov = [max(a, b) for a, b in zip(cov, _coverage(both, reads, k))]
    at_k, tied, none = cov
    assert at_k >= 2 and tied >= 2 and none >= 2, cov


def test_barcode_scan_partial_second_word(lib, tmp_path_factory):
    """45 barcodes on the forward primer: two 32-barcode words, the second partly filled"""
    pan, (pf, sf) = _panel(tmp_path_factory, "bs_two_words", 8, 45, 3, seed=77)
    reads = _reads(pan, 2, seed=78)
    for fl in (dict(index_edit_distance=2), dict(index_edit_distance=2, trim="tails"), dict(index_edit_distance=3)):
        both = Both(pf, sf, **fl)
        both.assert_hits_equal(reads, f"two words {fl}")
        both.assert_ops_equal(reads, f"two words {fl}")
    assert min(_coverage(both, reads, 3)) >= 2


def test_barcode_scan_m17_control(lib, tmp_path_factory):
    """17 nt: above the bit-sliced scans' 16 rows, the per-barcode path"""
    pan, (pf, sf) = _panel(tmp_path_factory, "bs_m17", 17, 6, 4, seed=17)
    reads = _reads(pan, 3, seed=18)
    for fl in (dict(index_edit_distance=3), dict(index_edit_distance=3, trim="tails")):
        both = Both(pf, sf, **fl)
        both.assert_hits_equal(reads, f"m17 {fl}")
        both.assert_ops_equal(reads, f"m17 {fl}")
