"""The padded barcode scan of the demux kernel's lean mode (smx_barcode_core.h, bitsliced_shw_pad: the bit-sliced diagonal
automaton) on the GPU, at the smallest shapes where it can go wrong: one panel per padded height and its lower neighbour
(barcodes of 4, 8, 9, 12, 13 and 16 nt), k = 0..3 on the default-flags (k = 3) and the generic kernels, k = 4 on the BSV = 2
kernel, and 1, 32 and 33 barcodes per primer (a full word; a second word holding one barcode).

Reads are built explicitly around one primer pair: the barcode with exactly d = 0..k+1 edits, barcodes whose best alignment
ends at each of the 2k + 1 live columns (0..k bases deleted from / inserted into the middle), ties between two barcodes one
substitution apart, N and R inside the barcode, and reads cut by the read end at every position from the barcode's first
base to three bases past its last, so that every ncol from 0 to m + k reaches the scan.  Lean hit tables and write
operations are compared with the oracle, and the oracle's hit tables must show that each case reached its edges: hits at
exactly k, tied hits (panels with two barcodes per primer or more), and hits with no barcode within k."""
import os
import random

import pytest

from parity_utils import Both, tmp_panel

pytestmark = pytest.mark.gpu

LENGTHS = (4, 8, 9, 12, 13, 16)
WORDS = (1, 32, 33)


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
    """n distinct random barcodes of length m; the second differs from the first in one position (ties)"""
    out = []
    while len(out) < n:
        if len(out) == 1:
            p = rng.randrange(m)
            b = out[0][:p] + rng.choice([c for c in "ACGT" if c != out[0][p]]) + out[0][p + 1:]
        else:
            b = "".join(rng.choice("ACGT") for _ in range(m))
        if b not in taken:
            taken.add(b)
            out.append(b)
    return out


def _panel(tmp_path_factory, name, m, nb, seed):
    from specimux_amd import synth
    rng = random.Random(seed)
    taken = set()
    f = _barcodes(rng, nb, m, taken)
    taken |= {synth.revcomp(b) for b in f}   # no reverse barcode equal to a forward one
    r = [synth.revcomp(b) for b in _barcodes(rng, nb, m, taken)]
    pan = synth.Panel([("ITS", "FWD", synth.ITS1F, "ITS4", synth.ITS4)], f, r)
    return pan, tmp_panel(tmp_path_factory, pan, name)


def _edited(rng, b, d):
    """b with exactly d edit operations (substitution, insertion, deletion) anywhere"""
    s = list(b)
    for _ in range(d):
        op = rng.randrange(3) if s else 1
        pos = rng.randrange(len(s)) if s else 0
        if op == 0:
            s[pos] = rng.choice([c for c in "ACGT" if c != s[pos]])
        elif op == 1:
            s.insert(pos, rng.choice("ACGT"))
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

    def either(name, edit):
        b1, b2 = rng.choice(f), rng.choice(r)
        add(name + "f", edit(b1), b2) if rng.random() < 0.5 else add(name + "r", b1, edit(b2))

    # exactly d edit operations, d = 0..k+1, on either barcode
    for d in range(k + 2):
        for _ in range(20):
            either(f"d{d}", lambda b: _edited(rng, b, d))
    # the best alignment ends at each of the 2k + 1 live columns: j bases deleted from / inserted into the middle; the read
    # goes on with random bases (lead / trail), so the row of the last barcode position is long enough on both sides
    for j in range(1, k + 1):
        h = m // 2
        for _ in range(6):
            either(f"del{j}", lambda b: b[:h] + b[h + j:] if j < m else b)
            either(f"ins{j}", lambda b: b[:h] + rnd(j) + b[h:])
    # ties: the position where the first two barcodes of a side differ set to N, or to a third letter
    if len(f) >= 2:
        for side, (x, y) in enumerate(((f[0], f[1]), (r[0], r[1]))):
            p = next(i for i in range(m) if x[i] != y[i])
            third = next(c for c in "ACGT" if c not in (x[p], y[p]))
            for c in ("N", third, "N", third):
                t = x[:p] + c + x[p + 1:]
                add("tie", t, rng.choice(r)) if side == 0 else add("tie", rng.choice(f), t)
    # N and R inside the barcode
    for c in "NR":
        for _ in range(6):
            either("iupac", lambda b, c=c, q=rng.randrange(m): b[:q] + c + b[q + 1:])
    # the read starts / ends inside the barcode or up to three bases (k + 1 if larger) past it: every ncol from 0 to m + k
    for cut in 2 * list(range(0, m + max(k + 1, 3) + 1)):
        b1, b2 = rng.choice(f), rng.choice(r)
        pad = max(k + 1, 3)
        add("cutf", (rnd(pad) + b1)[-cut:] if cut else "", b2, lead="", flip=False)
        add("cutr", b1, (b2 + rnd(pad))[:cut] if cut else "", trail="", flip=False)
        add("cutx", (rnd(pad) + b1)[-cut:] if cut else "", b2, lead="", flip=True)
    # no barcode anywhere near: primers with random flanks
    for _ in range(8):
        add("none", rnd(m), synth.revcomp(rnd(m)))
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


def _both_under(env, pf, sf, first, **flags):
    """parity_utils.Both compiled under the given switches (a panel reads them once, on its first batch)"""
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        both = Both(pf, sf, **flags)
        both.product_ops(first)
        return both
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _words(m, k):
    """barcodes per primer of the (m, k) case: every length meets 1, 32 and 33 over its k; the 13- and 16-row scans at the
    default k = 3, and the k = 4 scan at 13 nt, run all three"""
    if (k == 3 and m in (13, 16)) or (k == 4 and m == 13):
        return WORDS
    return (WORDS[(LENGTHS.index(m) + k) % 3],)


GRID = [(k, m, nb) for k in (0, 1, 2, 3) for m in LENGTHS for nb in _words(m, k)] + \
       [(4, m, nb) for m in LENGTHS if m > 4 for nb in _words(m, 4)]


@pytest.mark.parametrize("k,m,nb", GRID, ids=lambda v: str(v))
def test_barcode_automaton_edges(lib, tmp_path_factory, k, m, nb):
    pan, (pf, sf) = _panel(tmp_path_factory, f"ba_k{k}_m{m}_n{nb}", m, nb, seed=7000 + 100 * k + 10 * m + nb)
    reads = _reads(pan, k, seed=9000 + 100 * k + 10 * m + nb)
    assert 100 <= len(reads) <= 400, len(reads)
    flags = dict(index_edit_distance=k)
    if m - k < 2 or k == 0:   # the prefilter needs m - k >= 2, and at k = 0 its exact set drops the N reads of the ties
        flags["disable_prefilter"] = True
    # k <= 3: the kernel the flags select (default-flags at k = 3 with <= 32 barcodes per primer) and the generic one;
    # k = 4: the BSV = 2 kernel, which has no default-flags instantiation
    envs = [{}, {"SMX_NO_SPECIALISE": "1"}] if k <= 3 else [{}]
    both = None
    for env in envs:
        both = _both_under(env, pf, sf, reads[:1], **flags)
        both.assert_hits_equal(reads, f"k={k} m={m} nb={nb} {env}", lean=True)
        both.assert_ops_equal(reads, f"k={k} m={m} nb={nb} {env}")
    at_k, tied, none = _coverage(both, reads, k)
    assert at_k >= 2 and none >= 2 and (tied >= 2 or nb == 1), (at_k, tied, none)
