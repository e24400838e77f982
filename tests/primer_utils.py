"""Panels, constructed reads and a census for the demux kernel's per-read primer search (primer_item in smx_demux_tile.h, fed
by prescan_decode).  Plain Python; everything here is computed with the oracle alone.

The synthetic reads of specimux_amd.synth put the primer behind a 0-30 nt tail and a barcode, so nearly every match ends
in the window's last three 16-column chunks, and the synthetic panels stop at 31-nt primers (one 40-nt one).  Here the
primer length sits at the word-size edges (31, 32, 33, 63, 64 nt), the panels that make the whole search fall back (five
degenerate letters, SMX_NO_PRESCAN, one long primer among eight) are built, and the reads sweep the primer over every
window column, cut it at the window's inner edge, repeat it, damage it by exactly k and k + 1 edits, shorten the read
through every end_geom case and put non-ACGT bytes inside the window.

Everything is built in the SEARCH FRAME: match_one_end looks for primer_rc in the last search_len bases of q, where q is
the read (end 'B') or its reverse complement (end 'A').  A read is rc(tailF) + insert + tailR with
tail = V + rc(barcode) + pad: V is a variant of (an ACGT instance of) primer_rc, so V's last base lies in window column
S - 1 - len(pad) - len(barcode).  In the read this is pad(x) + b1 + P' + insert + rc(Q') + rc(b2) + pad(y) with
P' = rc(VF), rc(Q') = VR, x = y.

`census` labels every (read, primer, end) from the oracle's hit table; tests/test_primer_cases_cpu.py asserts that each
cell holds enough of every label, tests/test_primer_cases_gpu.py compares the kernel with the oracle on all the reads."""
import os
import random
import re
from collections import Counter

from oracle import edlib_semantics as E
from oracle import specimux_oracle as O
from specimux_amd import synth

# 64 nt of the 18S end / ITS1 start that ITS1F (its first 22 nt) primes into
LONG64 = "CTTGGTCATTTAGAGGAAGTAAAAGTCGTAACAAGGTTTCCGTAGGTGAACCTGCGGAAGGATC"
DEG5 = "GAYGARMGWGATCAYTTYGGKAC"      # Y, R, M, W, K: five distinct degenerate letters
BC_LEN = 13
MIN_HITS, MIN_READS = 4, 8
assert len(LONG64) == 64 and LONG64[:22] == synth.ITS1F
assert LONG64[:33] == "CTTGGTCATTTAGAGGAAGTAAAAGTCGTAACA"

_IUPAC = dict(synth._IUPAC)


def _one_pair(fwd, rev=synth.ITS4):
    f, r = synth.make_barcodes(8, 6, length=BC_LEN, min_dist=6, seed=7)
    return synth.Panel([("ITS", "FWD", fwd, "REV", rev)], f, r)


def _c3_m33():
    pan = synth.panel_c3()
    pools = [(pool, fn, LONG64[:33] if i == 0 else fs, rn, rs) for i, (pool, fn, fs, rn, rs) in enumerate(pan.pools)]
    return synth.Panel(pools, pan.fwd, pan.rev, shared_rev=pan.shared_rev)


PANELS = {
    "m22": lambda: _one_pair(synth.ITS1F), "m31": lambda: _one_pair(LONG64[:31]), "m32": lambda: _one_pair(LONG64[:32]),
    "m33": lambda: _one_pair(LONG64[:33]), "m63": lambda: _one_pair(LONG64[:63]), "m64": lambda: _one_pair(LONG64),
    "m32_rev": lambda: _one_pair(synth.ITS1F, LONG64[:32]), "m64_rev": lambda: _one_pair(synth.ITS1F, LONG64),
    "deg5": lambda: _one_pair(DEG5), "c3_m33": _c3_m33, "c3": synth.panel_c3,
}

# (panel, search_len, environment, the path of primer_item the cell is meant to reach)
PRESCAN_CELLS = [("m22", 16), ("m22", 80), ("m22", 160), ("m22", 256), ("m31", 256)]
BASE_CELLS = [
    ("m22", 16, {}, "prescan<0>"), ("m22", 80, {}, "prescan<5>"), ("m22", 160, {}, "prescan<10>"), ("m22", 256, {}, "prescan<0>"),
    ("m22", 84, {}, "unrolled u32"), ("m22", 83, {}, "generic u32"), ("m31", 256, {}, "prescan<0>"),
    ("m32", 80, {}, "unrolled u32"), ("m32", 83, {}, "generic u32"), ("m32_rev", 80, {}, "unrolled u32"),
    ("m32_rev", 83, {}, "generic u32"), ("m33", 80, {}, "generic u64"), ("m33", 256, {}, "generic u64"),
    ("m63", 80, {}, "generic u64"), ("m63", 256, {}, "generic u64"), ("m64", 80, {}, "generic u64"),
    ("m64", 256, {}, "generic u64"), ("m64_rev", 80, {}, "generic u64"), ("m64_rev", 256, {}, "generic u64"),
    ("deg5", 80, {}, "unrolled u32"), ("c3_m33", 80, {}, "generic u64"), ("c3_m33", 256, {}, "generic u64"),
    ("c3", 80, {"SMX_NO_PRESCAN": "1"}, "unrolled u32"),
]
VARIANT_CELLS = [(p, S, {"SMX_NO_PRESCAN": "1"}, "unrolled u32") for p, S in PRESCAN_CELLS] + \
                [(p, S, {"SMX_COMPACT_ITEMS": "120"}, f"prescan<{ {80: 5, 160: 10}.get(S, 0)}>") for p, S in PRESCAN_CELLS]
CELLS = BASE_CELLS + VARIANT_CELLS
CENSUS_CELLS = sorted({(p, S) for p, S, _e, _w in CELLS}, key=lambda c: (list(PANELS).index(c[0]), c[1]))


def cell_id(cell):
    p, S, env, _w = cell
    return f"{p}-S{S}" + "".join("-" + k[4:].lower() for k in env)


# ------------------------------------------------------------------ which path a panel takes (restated from the library)
def _header_constant(name):
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "specimux_amd", "csrc", "smx_prescan_core.h")) as fh:
        return int(re.search(rf"constexpr int {name} = (\d+);", fh.read()).group(1))


def expected_path(primers, S, env, maxrows=31, maxsym=8):
    """The path primer_item takes for a clean read of at least S bases, from the panel's primers alone:
    smx_panel_create (pre_ok, use64) and prescan_build_desc (smx_prescan_core.h) restated.  pre_ok: SMX_NO_PRESCAN unset,
    every primer of at most PRE_MAXROWS = 31 nt, S a multiple of 16 in 16..256, and per primer at most PRE_MAXSYM - 4 = 4
    distinct letters (as sets of A/C/G/T) besides the four bases.  use64: the longest primer exceeds 32 nt.  Without the
    prescan, 32-bit words and S % 4 == 0 give the unrolled scan, everything else the generic whole-window loop."""
    maxm = max(len(p) for p in primers)

    def fits(p):
        sets = {frozenset(_IUPAC[c]) for c in O.revcomp(p)} | {frozenset(b) for b in "ACGT"}
        return len(p) <= maxrows and len(sets) <= maxsym
    pre_ok = "SMX_NO_PRESCAN" not in env and maxm <= maxrows and 16 <= S <= 256 and S % 16 == 0 and all(fits(p) for p in primers)
    if pre_ok:
        return f"prescan<{ {80: 5, 160: 10}.get(S, 0)}>"
    if maxm > 32:
        return "generic u64"
    return "unrolled u32" if S % 4 == 0 else "generic u32"


# ------------------------------------------------------------------ constructed reads
def _other(rng_base, *avoid):
    """The first base after rng_base in ACGT order that none of the (possibly degenerate) letters in avoid matches."""
    bad = set("".join(_IUPAC.get(a, a) for a in avoid))
    for i in range(1, 5):
        b = "ACGT"[("ACGT".index(rng_base) + i) % 4]
        if b not in bad:
            return b
    raise ValueError(avoid)


def _sub(inst, pat, pos):
    s = list(inst)
    for p in pos:
        s[p] = _other(inst[p], pat[p])
    return "".join(s)


def _spread(m, n):
    return [((2 * i + 1) * m) // (2 * n) for i in range(n)]


def variants(pat, k, rng):
    """Search-frame texts for the pattern pat = primer_rc (IUPAC): an ACGT instance and its damaged forms."""
    inst = "".join(rng.choice(_IUPAC[c]) for c in pat)
    m = len(pat)
    return {
        "exact": inst,
        "sub_last": _sub(inst, pat, [0]),                 # the primer's last base = the pattern's first
        "del_mid": inst[:m // 2] + inst[m // 2 + 1:],
        "k_edits": _sub(inst, pat, _spread(m, k)),
        "k1_edits": _sub(inst, pat, _spread(m, k + 1)),
        "tandem": inst + inst,
        "rep6": inst[0] * 6 + inst,                        # the primer followed by six copies of its own last base
        # the pattern's last base once more behind a substituted one: ending on the substitution and ending one column
        # later (the substitute read as an insertion) cost one edit each -> two adjacent optimal ends
        "adjacent": inst[:-1] + _other(inst[-1], pat[-1], pat[-2]) + inst[-1],
        # the last base in place of the one before it: a substitution (ending in the last column) or a deletion (ending
        # one column earlier), one edit each; unlike `adjacent` it is no longer than the primer (the 16-column window)
        "adjacent2": inst[:-2] + inst[-1] + inst[-1],
    }


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def sweep_x(S, ms, off):
    """Pad lengths of the column sweep: all of them up to S = 96; on wider windows those that put the primer's end in
    column 0, 1, 14 or 15 mod 16, every fifth one, and the ones that cut the primer at the window's inner edge."""
    if S <= 96:
        return list(range(S))
    xs = set(range(0, S, 5))
    for x in range(S):
        e = S - 1 - off - x
        if e >= 0 and e % 16 in (0, 1, 14, 15):
            xs.add(x)
    for m in ms:
        for c in (0, 1, 2, 3, m // 2):
            if 0 <= S - off - m + c < S:
                xs.add(S - off - m + c)
    return sorted(xs)


def variant_x(S, m, off):
    """Pad lengths for the damaged primers: ends next to the read boundary and on both sides of every chunk / word edge."""
    ends = [S - 1 - off - x for x in (0, 1, 2, 4, 7)]
    ends += [c for c in (15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 95, 96, 127, 128, 129, 191, 192, 223, 224, 239, 240)]
    ends += [m - 1, m, m + 1]                                # the start in columns 0, 1, 2
    ends = sorted({e for e in ends if m - 1 <= e <= S - 1 - off})
    if len(ends) > 12:
        ends = sorted(set(ends[:3] + ends[-5:] + ends[3:-5][::max(1, (len(ends) - 8) // 4)][:4]))
    return [S - 1 - off - e for e in ends]


class Cell:
    """The constructed reads of one (panel, search_len): .reads = [(id, bases, quality)], .meta[id] = dict(dirty, sites)
    with sites = the (primer name, end) pairs a primer was planted at."""

    def __init__(self, name, S):
        self.name, self.S = name, S
        self.panel = PANELS[name]()
        self.rng = random.Random(f"{name}/{S}")
        self.reads, self.meta = [], {}
        self._build()

    def write(self, d):
        return self.panel.write(d)

    def primer_seqs(self):
        return [s for _p, _fn, fs, _rn, rs in self.panel.pools for s in (fs, rs)]

    # one read and its reverse complement
    def _add(self, tag, pool, vf, vr, x, bc=True, L=None, dirt=None, tail_L=False):
        rng, S = self.rng, self.S
        _pn, fn, _fs, rn, _rs = self.panel.pools[pool]
        n = len(self.reads)
        b1 = self.panel.fwd[n % len(self.panel.fwd)] if bc else ""
        b2 = self.panel.rev[n % len(self.panel.rev)] if bc else ""
        head = O.revcomp(vf + O.revcomp(b1) + _rand(rng, x))
        tail = vr + O.revcomp(b2) + _rand(rng, x)
        ins = _rand(rng, 2 * S + 40 + rng.randrange(0, 30))
        s = head + ins + tail
        if dirt:
            s = dirt(s, x, len(b1), len(vf), len(vr))
        if L is not None:
            s = s[len(s) - L:] if tail_L and L else s[:L]
        for o in "fr":
            rid = f"{tag}_x{x}_{'b' if bc else 'n'}_{len(self.reads)}{o}"
            seq = s if o == "f" else O.revcomp(s)
            q = "".join(chr(33 + rng.randrange(3, 41)) for _ in seq)
            self.reads.append((rid, seq, q))
            a, b = ("A", "B") if o == "f" else ("B", "A")
            self.meta[rid] = dict(dirty=dirt is not None, sites={(fn, a), (rn, b)})

    def _build(self):
        S, pan = self.S, self.panel
        par = O.setup_params(O.load_panel(*_written(self)), search_len=S)
        V = []
        for _pn, _fn, fs, _rn, rs in pan.pools:
            V.append((variants(O.revcomp(fs), par.max_dist_primers[fs], self.rng),
                      variants(O.revcomp(rs), par.max_dist_primers[rs], self.rng), len(fs), len(rs)))
        npool = len(pan.pools)
        vf0, vr0, mf0, mr0 = V[0]
        # 1. column sweep of the exact primer: behind a barcode (pool 0), and flush with the pad (the pools in rotation)
        for bc in (True, False):
            off = BC_LEN if bc else 0
            for i, x in enumerate(sweep_x(S, {m for v in V for m in v[2:]}, off)):
                pool = 0 if bc else i % npool
                self._add("sweep", pool, V[pool][0]["exact"], V[pool][1]["exact"], x, bc)
        # 2. the damaged primers
        for pool in range(npool):
            vf, vr, mf, mr = V[pool]
            for kind in ("sub_last", "del_mid", "k_edits", "k1_edits", "rep6", "adjacent", "adjacent2"):
                xs = sorted(set(variant_x(S, mf, BC_LEN) + variant_x(S, mr, BC_LEN)))
                if npool > 1:
                    xs = xs[pool % 2::2][:4]
                for x in xs:
                    self._add(kind, pool, vf[kind], vr[kind], x, True)
                for x in (0, 1, 2):
                    if npool == 1 or x == pool % 3:
                        self._add(kind, pool, vf[kind], vr[kind], x, False)
        # 3. the primer twice in a row, swept: two optimal ends a primer length apart, in one word and in two
        step = 1 if S <= 96 else 3
        for bc in (True, False):
            off = BC_LEN if bc else 0
            for i, x in enumerate(range(0, S, step)):
                pool = i % npool
                if 2 * min(V[pool][2:]) + off + x <= S:
                    self._add("tandem", pool, V[pool][0]["tandem"], V[pool][1]["tandem"], x, bc)
        # 4. the end_geom cases: the head (tail) of a construct cut to L bases
        lens = []
        for m in sorted({mf0, mr0}):
            lens += [m + BC_LEN, m, m - 1]
        lens += [S + 1, S, S - 1, S - 2, S // 2 + 5, S // 2 + 2, S // 2 + 1, S // 2, S // 2 - 1, 1, 0]
        for L in sorted({l for l in lens if l >= 0}):
            for x, bc in ((0, True), (2, True), (0, False), (1, False), (3, False)):
                self._add(f"len{L}", 0, vf0["exact"], vr0["exact"], x, bc, L=L)
                self._add(f"len{L}t", 0, vf0["exact"], vr0["exact"], x, bc, L=L, tail_L=True)
        # 5. dirty reads: one byte that is not upper-case ACGT inside the window (no U: a documented divergence)
        def at(where, ch):
            def put(s, p):
                return s[:p] + (s[p].lower() if ch == "lower" else ch) + s[p + 1:]

            def dirt(s, x, nb, nvf, nvr):
                off = {"primer": lambda nv: nb + nv // 3, "barcode": lambda nv: nb // 2, "insert": lambda nv: nb + nv + 5}[where]
                return put(put(s, x + off(nvf)), len(s) - 1 - x - off(nvr))     # on the forward and on the reverse primer's side
            return dirt
        dirts = [("lc", at("primer", "lower")), ("N", at("primer", "N")), ("R", at("primer", "R")),
                 ("Nbc", at("barcode", "N")), ("X", at("insert", "X"))]
        for kind in ("exact", "sub_last", "k_edits", "k1_edits"):
            for dn, d in dirts:
                for x in (0, 3, max(0, S - BC_LEN - max(mf0, mr0) - 2)):
                    self._add(f"dirty_{dn}_{kind}", 0, vf0[kind], vr0[kind], x, True, dirt=d)
                if dn != "Nbc":
                    self._add(f"dirty_{dn}_{kind}", 0, vf0[kind], vr0[kind], 0, False, dirt=d)
        assert len({r[0] for r in self.reads}) == len(self.reads)


_FILES, _CELLS = {}, {}


def _written(cell):
    """Panel files of a cell's panel in a scratch directory of this process (the census and the read builder need the
    oracle's thresholds)."""
    import atexit
    import shutil
    import tempfile
    if cell.name not in _FILES:
        d = tempfile.mkdtemp(prefix=f"smx_primer_{cell.name}_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        _FILES[cell.name] = cell.panel.write(d)
    return _FILES[cell.name]


def cell(name, S):
    if (name, S) not in _CELLS:
        _CELLS[(name, S)] = Cell(name, S)
    return _CELLS[(name, S)]


# ------------------------------------------------------------------ the census
GEOM = ["L>=S", "L==S-1", "S/2<L<=S-2", "L<=S/2"]
LABELS = ["end_last_col", "start_first_col", "multi_adjacent", "multi_two_words", "d0", "d_eq_k", "d_eq_k_plus_1",
          "dirty_matched", "dirty_unmatched"] + GEOM
AT_LEAST_8 = {"d0", "d_eq_k", "d_eq_k_plus_1", "dirty_matched", "dirty_unmatched"}


def geom_class(L, S):
    return "L>=S" if L >= S else "L==S-1" if L == S - 1 else "S/2<L<=S-2" if 2 * L > S else "L<=S/2"


def target_of(L, S):
    """(q index of the primer target's first base as align_seq reports it, target length): alignment.py:37-40 with Python's
    slice semantics for a negative start."""
    if L >= S:
        return L - S, S
    if L == S - 1:
        return 0, L
    return L - S, min(L, S - L)


_TABLES = {}


def hit_table(cell_, par, panel, rec):
    key = (cell_.name, cell_.S, rec[0])
    if key not in _TABLES:
        _TABLES[key] = O.hit_table(par, panel, rec)
    return _TABLES[key]


def census(cell_, reads=None, only=None):
    """Counter over LABELS and ('end_chunk', c), from the oracle alone: O.hit_table, and for the near misses the oracle's
    aligner with the threshold lifted to the primer length.  Coordinates are relative to the target's first base.
    only: count this primer's alignments alone."""
    S = cell_.S
    panel = O.load_panel(*_written(cell_))
    par = O.setup_params(panel, search_len=S)
    counts = Counter()
    for rec in reads or cell_.reads:
        rid, s, _q = rec
        L = len(s)
        s0, T = target_of(L, S)
        meta = cell_.meta[rid]
        table = hit_table(cell_, par, panel, rec)
        for primer in panel.primers.values():
            if only is not None and primer.name != only:
                continue
            k, m = par.max_dist_primers[primer.primer], len(primer.primer)
            for end in "AB":
                h = table[(primer.name, end)]
                if h["pdist"] < 0:
                    if meta["dirty"] and (primer.name, end) in meta["sites"]:
                        counts["dirty_unmatched"] += 1
                    q = s if end == "B" else O.revcomp(s)
                    t = q[0 if L - S == -1 else L - S:L]         # align_seq's target (alignment.py:37-40)
                    if t and E.align(primer.primer_rc, t, E.HW, -1, iupac=True)["editDistance"] == k + 1:
                        counts["d_eq_k_plus_1"] += 1
                    continue
                ends = [e - s0 for _a, e in h["locs"]]
                st, e = h["locs"][0][0] - s0, ends[0]
                assert 0 <= st <= e < T, (rid, primer.name, end, h, s0, T)
                counts[("end_chunk", e // 16)] += 1
                counts["end_last_col"] += e == T - 1
                counts["start_first_col"] += st == 0
                if len(ends) >= 2:
                    counts["multi_adjacent"] += any(b - a == 1 for a, b in zip(ends, ends[1:]))
                    counts["multi_two_words"] += len({x // 32 for x in ends}) >= 2
                counts["d0"] += h["pdist"] == 0
                counts["d_eq_k"] += h["pdist"] == k
                counts[geom_class(L, S)] += 1
                counts["dirty_matched"] += meta["dirty"]
    return counts


def cannot(cell_):
    """{label: reason} of what cannot occur in a cell.  need = min over the panel's primers of m - k: an alignment within
    k edits spends at least m - k target columns, so it ends in column need - 1 or later and needs a target that long."""
    S = cell_.S
    panel = O.load_panel(*_written(cell_))
    par = O.setup_params(panel, search_len=S)
    need = min(len(p.primer) - par.max_dist_primers[p.primer] for p in panel.primers.values())
    out = {}
    for c in range((S + 15) // 16):
        if 16 * c + 15 < need - 1:
            out[("end_chunk", c)] = f"a match ends in column {need - 1} or later"
    longest = {"L>=S": S, "L==S-1": S - 1, "S/2<L<=S-2": S - (S // 2 + 1), "L<=S/2": S // 2}
    for g, t in longest.items():
        if t < need:
            out[g] = f"the longest target of the class has {t} columns, a match needs {need}"
    if S < 64:
        out["multi_two_words"] = "the window has fewer than 64 columns"
    if all(len(p.primer) > S for p in panel.primers.values()):
        out["d0"] = "every primer is longer than the window"
    return out
