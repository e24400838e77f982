"""Hand-written panels, constructed reads and a census for the demux scorer (phase 4 of the demux kernel: score_fast,
score_general, emit_op, specimen_exact, specimens_for).  Plain Python; everything here is computed with the oracle alone.

The synthetic panels of specimux_amd.synth are full forward x reverse barcode grids with one named primer pair per pool;
on them most of the scorer's case analysis cannot be reached.  The panels below are sparse sheets with wildcards, close
primer variants that both match one window, duplicate barcode pairs, a shared primer sequence and more than 32 primer
pairs, and the reads are a cross product over primer text x barcode text x orientation plus a few special families.
`situation` names the scorer branch a read lands in; tests/test_scorer_cases_cpu.py checks that every reachable branch
holds at least MIN_READS reads under every flag set, tests/test_scorer_cases_gpu.py compares the kernel with the oracle."""
import itertools
import os
import random
from collections import Counter

from oracle import specimux_oracle as O

MIN_READS = 8
HEADER = "SampleID\tPrimerPool\tFwIndex\tFwPrimer\tRvIndex\tRvPrimer\n"

# ------------------------------------------------------------------ primers
FA1 = "CTTGGTCATTTAGAGGAAGTAA"        # ITS1F, k = 7
FA2 = "CTTGGACATTTAGACGAAGTAA"        # two substitutions away: a window that carries one matches both
FAM = "CTTGGACATTTAGAGGAAGTAA"        # one substitution from each
RA1 = "TCCTCCGCTTATTGATATGC"          # ITS4, k = 6
RA2 = "TCCTGCGCTTATTTATATGC"
RAM = "TCCTGCGCTTATTGATATGC"
FB = "ACCCGCTGAACTTAAGC"              # LR0R, k = 5
WIDE_FWD = ["CGATTCAAATGACGGCAGCA", "GGCCGGGAGTCCCTGAGAGG", "CTTGTTCCGGAAATGTGCCA", "AAGAGGAGGGCTAGCTGCGT",
            "CGAGATCGGGATCTCAAAAC", "CATCGAAGTCTCCTTTACTT", "ATTATCCGGTGTCGGTTAGC", "ATCGACTTTTCACCAGATTC"]
WIDE_FWD.append("ATCGTCTTTTCACCAGTTTC")   # W9 = W8 with two substitutions: candidates 56.. and 64.. both match a W8 window
WIDE_REV = ["TACGCCCGTGGACAGAATTA", "CTGGCCAAGTGTTTCGGGCT", "ACCGGCGAATCGGGCGAAAG", "TGGTTAGCTGTTACATGGAG"]

# ------------------------------------------------------------------ barcodes (13 nt, min pairwise edit distance 5 -> k_idx 3)
# F0, F1, F2 are one centre (F3WAY) with positions 1-3, 4-6, 7-9 substituted: mutually at Hamming distance 6, each at 3
# from the centre.  F2WAY takes three of the six positions where F0 and F1 differ from F1: at 3 from F0 and F1, at 7 or
# more from every other barcode (also as a prefix alignment anchored at the primer, which is what the search runs).  Same for R*.
F = ["CCCGCAACCCTAT", "CGTCGTCCCCTAT", "CGTCCAAGAGTAT", "CCAATCCTTGGTC", "CAGGTCGCGGACG", "CAGGCGATGTGTC"]
R = ["CTACTTAGAATTA", "CAGTAGCGAATTA", "CAGTTTACTTTTA", "TACACCGAATGCT", "CCTTTTAAGAAAA", "GCTCACACGTAGG"]
F3WAY, F2WAY = "CGTCCAACCCTAT", "CGCGGACCCCTAT"
R3WAY, R2WAY = "CAGTTTAGAATTA", "CTGCTGCGAATTA"


def _sub(s, *pos):
    s = list(s)
    for p in pos:
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
    return "".join(s)


# a window only the first variant matches: FA1 + 6 substitutions is at 6 <= 7 from FA1 and at 8 from FA2 (k = 7); RA1 + 5 at
# 5 <= 6 from RA1 and at 7 from RA2 (k = 6) -- the way to ONE full candidate on the panels that hold both variants
FA1X = _sub(FA1, 1, 3, 8, 11, 17, 20)
RA1X = _sub(RA1, 1, 7, 10, 16, 18)


def barcode_texts(B, two, three):
    """label -> text found next to the primer.  `None` = nothing there."""
    return {"b0": B[0], "b1": B[1], "b2": B[2], "b3": B[3], "b4": B[4], "b5": B[5],
            "b0e1": _sub(B[0], 11), "b0e2": _sub(B[0], 0, 11), "b3d1": B[3][:10] + B[3][11:], "b3e2": _sub(B[3], 0, 12),
            "two": two, "three": three, "b0n": B[0][:5] + "N" + B[0][6:], "absent": ""}


FTEXT, RTEXT = barcode_texts(F, F2WAY, F3WAY), barcode_texts(R, R2WAY, R3WAY)
INS = "ACGGTTCAGGCTAACGTTAGC" * 8


class HandPanel:
    def __init__(self, name, primers, rows, fwd_texts, rev_texts, core_primers, seed, solo=None):
        self.name, self.primers, self.rows = name, primers, rows
        self.fwd_texts, self.rev_texts = fwd_texts, rev_texts   # label -> primer text a read may carry (None: no primer)
        self.core_primers = core_primers                        # (fwd label, rev label) variants every core combination gets
        self.seed = seed
        self.solo = solo    # the core primer variant under which a read has ONE full candidate (its tied reads get more flanks)

    def write(self, d):
        pf, sf = os.path.join(d, "primers.fasta"), os.path.join(d, "specimens.txt")
        with open(pf, "w") as fh:
            for name, pools, pos, seq in self.primers:
                fh.write(f">{name} pool={pools} position={pos}\n{seq}\n")
        with open(sf, "w") as fh:
            fh.write(HEADER)
            for row in self.rows:
                fh.write("\t".join(row) + "\n")
        return pf, sf


def _rows(spec):
    return [(f"s{i + 1:02d}", pool, F[int(fb)], fp, R[int(rb)], rp) for i, (pool, fb, fp, rb, rp) in enumerate(spec)]


# (pool, forward barcode, forward primer, reverse barcode, reverse primer)
_MULTI_ROWS = _rows([
    ("A", 0, "FA1", 0, "RA1"), ("A", 1, "FA1", 0, "RA1"), ("A", 0, "*", 1, "RA1"), ("A", 1, "FA2", 1, "*"),
    ("A", 2, "-", 2, "-"), ("A", 0, "FA1", 2, "RA2"), ("A", 2, "FA1", 0, "RA1"),
    ("A", 3, "FA1", 3, "RA1"), ("A", 3, "FA1", 3, "RA1"),        # one barcode pair, two ids, the same primers
    ("A", 4, "FA1", 4, "RA1"), ("A", 4, "FA2", 4, "RA2"),        # one barcode pair, two ids, different primers
    ("B", 3, "FB", 3, "RA1"),                                    # the (3, 3) pair again, in the other pool
    ("B", 4, "FB", 0, "RA1"),
    ("A", 5, "FA1", 5, "RA1"),                                   # 5 pairs with 5 only: "a barcode the sheet pairs with nothing"
    ("A", 2, "FA1", 1, "RA1"),                                   # makes the three-way x two-way tie hold 5 specimens
])
_A_TEXTS_F = {"FA1": FA1, "FA2": FA2, "FAM": FAM, "FA1X": FA1X, "FB": FB, "none": None}
_A_TEXTS_R = {"RA1": RA1, "RA2": RA2, "RAM": RAM, "RA1X": RA1X, "none": None}

PANELS = {}
PANELS["multi"] = HandPanel(
    "multi",
    [("FA1", "A", "forward", FA1), ("FA2", "A", "forward", FA2), ("RA1", "A,B", "reverse", RA1),
     ("RA2", "A", "reverse", RA2), ("FB", "B", "forward", FB)],
    _MULTI_ROWS, _A_TEXTS_F, _A_TEXTS_R,
    [("FA1", "RA1"), ("FA2", "RA2"), ("FAM", "RAM"), ("FA1X", "RA1X"), ("FB", "RA1")], 11, solo=("FA1X", "RA1X"))

PANELS["two_pairs"] = HandPanel(
    "two_pairs",
    [("FA1", "A", "forward", FA1), ("FA2", "A", "forward", FA2), ("RA1", "A", "reverse", RA1)],
    _rows([("A", 0, "FA1", 0, "RA1"), ("A", 1, "FA1", 0, "RA1"), ("A", 0, "*", 1, "RA1"), ("A", 1, "FA2", 1, "RA1"),
           ("A", 2, "-", 2, "-"), ("A", 2, "FA1", 0, "RA1"), ("A", 3, "FA1", 3, "RA1"), ("A", 3, "FA1", 3, "RA1"),
           ("A", 4, "FA1", 4, "RA1"), ("A", 4, "FA2", 4, "RA1"), ("A", 5, "FA1", 5, "RA1"), ("A", 2, "FA1", 1, "RA1")]),
    {k: v for k, v in _A_TEXTS_F.items() if k != "FB"}, {"RA1": RA1, "RAM": RAM, "none": None},
    [("FA1", "RA1"), ("FA2", "RA1"), ("FAM", "RAM"), ("FA1X", "RA1"), ("FA1X", "RAM")], 12, solo=("FA1X", "RA1"))

PANELS["one_pair_sparse"] = HandPanel(
    "one_pair_sparse",
    [("FA1", "A", "forward", FA1), ("RA1", "A", "reverse", RA1)],
    _rows([("A", 0, "FA1", 0, "RA1"), ("A", 1, "FA1", 0, "RA1"), ("A", 0, "FA1", 1, "RA1"), ("A", 2, "FA1", 2, "RA1"),
           ("A", 2, "FA1", 0, "RA1"), ("A", 3, "FA1", 3, "RA1"), ("A", 3, "*", 3, "-"), ("A", 4, "FA1", 4, "RA1"),
           ("A", 5, "FA1", 5, "RA1")]),
    {"FA1": FA1, "FAM": FAM, "FA1X": FA1X, "none": None}, {"RA1": RA1, "RAM": RAM, "RA1X": RA1X, "none": None},
    [("FA1", "RA1"), ("FAM", "RAM"), ("FA1X", "RA1X"), ("FA1", "RAM")], 13)

_WF = [f"W{i + 1}" for i in range(9)]
_WR = [f"X{i + 1}" for i in range(4)]
PANELS["wide"] = HandPanel(
    "wide",
    [(n, "W", "forward", s) for n, s in zip(_WF, WIDE_FWD)] + [(n, "W", "reverse", s) for n, s in zip(_WR, WIDE_REV)],
    _rows([("W", 0, "*", 0, "*"), ("W", 1, "W8", 0, "-"), ("W", 0, "W9", 1, "X4"), ("W", 1, "*", 1, "X1"),
           ("W", 2, "-", 2, "-"), ("W", 2, "W8", 0, "X4"), ("W", 3, "W1", 3, "X1"), ("W", 3, "W9", 3, "X4"),
           ("W", 3, "W9", 3, "X4"), ("W", 4, "W8", 4, "*"), ("W", 5, "W5", 5, "X2"), ("W", 1, "*", 0, "*"),
           ("W", 2, "W1", 0, "X1"), ("W", 0, "W1", 1, "-")]),
    {"W8": WIDE_FWD[7], "W9": WIDE_FWD[8], "W8M": WIDE_FWD[7][:3] + WIDE_FWD[8][3] + WIDE_FWD[7][4:], "W1": WIDE_FWD[0],
     "W5": WIDE_FWD[4], "none": None},
    {"X4": WIDE_REV[3], "X1": WIDE_REV[0], "X2": WIDE_REV[1], "none": None},
    [("W8", "X4"), ("W9", "X4"), ("W8M", "X4"), ("W1", "X1"), ("W9", "X1")], 14, solo=("W1", "X1"))

PANELS["same_sequence"] = HandPanel(
    "same_sequence",
    # FA1 and FA1B are one sequence under two names (Q5): the first one a specimen row registers serves the sequence, a
    # row that names the other one can never be matched (`p1 in p1s` is object identity, databases.py:224,241)
    [("FA1", "A", "forward", FA1), ("FA1B", "A", "forward", FA1), ("RA1", "A", "reverse", RA1)],
    _rows([("A", 0, "FA1", 0, "RA1"), ("A", 1, "FA1B", 0, "RA1"), ("A", 0, "FA1B", 1, "RA1"), ("A", 2, "*", 2, "RA1"),
           ("A", 2, "FA1", 0, "RA1"), ("A", 3, "FA1B", 3, "RA1"), ("A", 3, "FA1", 3, "RA1"), ("A", 4, "FA1", 4, "RA1"),
           ("A", 1, "FA1", 1, "RA1"), ("A", 5, "FA1B", 5, "RA1"), ("A", 1, "FA1", 0, "RA1"), ("A", 4, "*", 4, "RA1")]),
    {"FA1": FA1, "FAM": FAM, "none": None}, {"RA1": RA1, "RAM": RAM, "none": None},
    [("FA1", "RA1"), ("FAM", "RAM"), ("FA1", "RAM"), ("FAM", "RA1")], 15)

# (forward barcode text, reverse barcode text) every panel's reads hold under each of its core primer variants, both ways round
CORES = [("b0", "b0"), ("b3", "b3"), ("b4", "b4"), ("b0", "b1"), ("b1", "b1"), ("b2", "b2"), ("b0", "b2"), ("b5", "b5"),
         ("two", "b0"), ("two", "b1"), ("three", "b0"), ("three", "three"), ("two", "two"), ("two", "b3"), ("three", "b4"),
         ("b0", "b3"), ("b5", "b0"), ("b3", "two"), ("two", "b2"), ("three", "b2"), ("b0", "two"), ("b0e1", "b0e2"),
         ("three", "two"), ("b1", "two"),
         ("b0", "absent"), ("absent", "b0"), ("two", "absent"), ("absent", "three"), ("b0n", "b0"), ("absent", "absent"),
         ("b3", "absent"), ("absent", "b3e2")]


def _structure(fb, fp, rb, rp, ins=INS, head="TTTT", tail="GGGG"):
    left = (head + FTEXT[fb] + fp) if fp else head
    right = (O.revcomp(rp) + O.revcomp(RTEXT[rb]) + tail) if rp else tail
    return left + ins + right


def make_reads(pan, n_sample=100):
    """Constructed reads of one panel: [(id, bases, quality)], about 600 at the most."""
    ft, rt = pan.fwd_texts, pan.rev_texts
    out = []
    # 1. the core combinations under every core primer variant, as read and reverse complemented; the tied ones once more
    #    with other flanks under the variant that leaves one full candidate
    for (fb, rb), (fp, rp) in itertools.product(CORES, pan.core_primers):
        flanks = [("TTTT", "GGGG")]
        if (fp, rp) == pan.solo and ("two" in (fb, rb) or "three" in (fb, rb)):
            flanks += [("ACAC", "TGTG"), ("G", "CA")]
        for k, (head, tail) in enumerate(flanks):
            s = _structure(fb, ft[fp], rb, rt[rp], head=head, tail=tail)
            for o in "fr":
                out.append((f"core{k}_{fb}_{rb}_{fp}_{rp}_{o}", s if o == "f" else O.revcomp(s)))
    # 2. a deterministic sample of the whole cross product
    cross = list(itertools.product(sorted(ft), sorted(rt), sorted(FTEXT), sorted(RTEXT), "fr"))
    for fp, rp, fb, rb, o in random.Random(pan.seed).sample(cross, min(n_sample, len(cross))):
        s = _structure(fb, ft[fp], rb, rt[rp])
        out.append((f"x_{fb}_{rb}_{fp}_{rp}_{o}", s if o == "f" else O.revcomp(s)))
    f_names, r_names = [k for k in ft if ft[k]], [k for k in rt if rt[k]]
    f1, r1 = ft[f_names[0]], rt[r_names[0]]
    # 3. the forward (reverse) structure at both ends: the orientation vote stays undecided, both orientations give a
    #    partial candidate -- two different barcodes (several groups), the same one (one group), tied ones, none at all
    for i, (a, b) in enumerate(BOTH_ENDS):
        fp, rp = ft[f_names[i % len(f_names)]], rt[r_names[i % len(r_names)]]
        ins = INS[:60 + 5 * (i % 8)]
        out.append((f"ff_{a}_{b}_{i}", "TTTT" + FTEXT[a] + fp + ins + O.revcomp(fp) + O.revcomp(FTEXT[b]) + "GGGG"))
        out.append((f"rr_{a}_{b}_{i}", "TTTT" + RTEXT[a] + rp + ins + O.revcomp(rp) + O.revcomp(RTEXT[b]) + "GGGG"))
    # 4. the whole structure both ways round in one read: a full candidate in either orientation, the as-read one first
    for i, (fa, ra, fb, rb) in enumerate(DUAL):
        fp = ft[f_names[i % min(2, len(f_names))]]
        s = (RTEXT[rb] + r1 + FTEXT[fa] + fp + INS[:60] + O.revcomp(r1) + O.revcomp(RTEXT[ra]) + O.revcomp(fp)
             + O.revcomp(FTEXT[fb]))
        out.append((f"dual_{fa}_{ra}_{fb}_{rb}_{i}", s))
    # 5. inside out: the reverse primer's site before the forward primer's -> every trim mode cuts to nothing (Q12)
    for j in range(10):
        s = "AC" * (j % 3) + O.revcomp(r1) + INS[:j] + f1 + "GT" * (j % 2)
        out.append((f"inout_{j}", s if j % 2 == 0 else O.revcomp(s)))
    # 6. reads of 30-79 nt: the two search windows overlap or cover the whole read
    for j, L in enumerate(range(30, 80, 3)):
        whole = FTEXT["b0"] + f1 + INS[:max(0, L - 68)] + O.revcomp(r1) + O.revcomp(RTEXT["b0"])
        out.append((f"short_whole_{L}", whole[:L] if j % 2 else whole[-L:]))
        half = ("TT" + FTEXT["b3"] + f1 + INS)[:L]
        out.append((f"short_fwd_{L}", half if j % 2 else O.revcomp(half)))
    # 7. one primer and nothing else (under the variant only one primer matches, where the panel has one)
    fx = ft[pan.solo[0]] if pan.solo else f1
    for j in range(10):
        s = "TTTTACCA"[j % 4:] + fx + INS[:70 + j]
        out.append((f"lone_{j}", s if j % 2 == 0 else O.revcomp(s)))
    assert len({rid for rid, _s in out}) == len(out)
    rng = random.Random(pan.seed + 100)
    return [(rid, s, "".join(chr(33 + rng.randrange(3, 41)) for _ in s)) for rid, s in out]


BOTH_ENDS = [("b0", "b1"), ("b1", "b2"), ("b3", "b4"), ("b2", "b0"), ("b4", "b0"), ("b0", "b3"), ("b1", "b3"), ("b2", "b4"),
             ("b5", "b0"), ("b0e1", "b3"),
             ("b0", "b0"), ("b3", "b3"), ("b1", "b1"), ("b4", "b4"), ("b0e1", "b0"), ("b0", "b0e2"), ("b2", "b2"), ("b5", "b5"),
             ("b3e2", "b3"), ("b3", "b3d1"),
             ("two", "b0"), ("three", "three"), ("two", "two"), ("b0", "three"), ("two", "b3"), ("three", "b1"), ("b2", "two"),
             ("b1", "three"), ("three", "b4"), ("b3", "two"),
             ("absent", "absent")] + [("absent", "absent")] * 9 + [("b0", "absent"), ("absent", "b3")]
DUAL = [("b0e1", "b0", "b0", "b0"), ("b0e2", "b0", "b0", "b0"), ("b0", "b0e1", "b0", "b0"), ("b0", "b0e2", "b0", "b0"),
        ("b0e1", "b0e1", "b0", "b0"), ("b3e2", "b3", "b3", "b3"), ("b3", "b3e2", "b3", "b3"), ("b3d1", "b3", "b3", "b3"),
        ("b0e2", "b0e2", "b0", "b0e1"), ("b4", "b4", "b4", "b4"),
        ("b0", "b3", "b0", "b0"), ("b0", "b0", "b0", "b3"), ("b5", "b0", "b3", "b3"), ("b3", "b3", "b5", "b0"),
        ("b0", "b3", "b3", "b3"), ("b3", "b3", "b0", "b3"), ("b4", "b0", "b0", "b0"), ("b0", "b0", "b4", "b0"),
        ("b0", "b3", "b5", "b0"), ("b3", "b0", "b4", "b4"),
        ("two", "b0", "b0", "b0"), ("b0", "b0", "two", "two"), ("three", "three", "b0", "b0"), ("b0", "b0", "three", "b0"),
        ("two", "b1", "b0", "b1"), ("b3", "b3", "two", "b0"), ("b0", "two", "b0", "b0"), ("three", "b2", "b2", "b2"),
        ("two", "b3", "b0", "b0"), ("b1", "b0", "two", "b0"),
        ("b0", "b0", "b0", "b0"), ("b3", "b3", "b3", "b3"), ("b0", "b0", "b1", "b0"), ("b2", "b2", "b0", "b1"),
        ("b1", "b0", "b1", "b0")]


# ------------------------------------------------------------------ flag sets
FLAG_SETS = {"default": dict(), "derep_none": dict(dereplicate="none"), "trim_tails": dict(trim="tails"),
             "trim_primers_derep_none": dict(trim="primers", dereplicate="none"), "no_preorient": dict(disable_preorient=True),
             "k5": dict(index_edit_distance=5)}


# ------------------------------------------------------------------ the census
SITUATIONS = ["0", "1-2/one", "1-2/several", "3-4/one/untied", "3-4/one/tied", "3-4/several/untied/one_group",
              "3-4/several/untied/several_groups", "3-4/several/tied", "5/one/untied/spec0", "5/one/untied/spec1",
              "5/one/tied/spec0", "5/one/tied/spec1", "5/one/tied/spec2-4", "5/one/tied/spec5up", "5/several/untied",
              "5/several/tied", "5/several:none", "5/several:shared", "5/several:late"]
PROPERTIES = ["multi_record", "trim_empty", "cand_twice", "multiple_untied"]


def _full_key(m):   # dereplicate_matches' sort key (demultiplex.py:371-378)
    return (m.b1d() + m.b2d(), m.p1d() + m.p2d(), m.p1.file_index + m.p2.file_index)


def classify(panel, cands):
    """Label of one read from its candidate list (find_candidates order): score class of the best list / one or several
    best candidates / untied or tied / groups or specimens.  Several full candidates add '+none' (a best candidate maps
    to no specimen), '+shared' (two candidates map to one specimen) and '+late' (a specimen group's winner by the
    dereplication key is not its first member)."""
    if not cands:
        return "0"
    best = O.select_best(cands)
    sc = O.score(best[0])
    n = "one" if len(best) == 1 else "several"
    if sc <= 2:
        return f"1-2/{n}"
    if sc <= 4:
        groups, tied = set(), False
        for m in best:
            d, bcs = ("forward", m.best_b1()) if m.b1 else ("reverse", m.best_b2())
            tied = tied or len(bcs) > 1
            groups.update((d, b) for b in bcs)
        if n == "one":
            return f"3-4/one/{'tied' if tied else 'untied'}"
        if tied:
            return "3-4/several/tied"
        return f"3-4/several/untied/{'one_group' if len(groups) == 1 else 'several_groups'}"
    per, tied = [], False
    for m in best:
        specs = []
        for b1 in m.best_b1():
            for b2 in m.best_b2():
                s = panel.specimen_for_exact(b1, b2, m.p1, m.p2)
                if s and s not in specs:
                    specs.append(s)
        tied = tied or len(m.best_b1()) * len(m.best_b2()) > 1
        per.append(specs)
    t = "tied" if tied else "untied"
    if n == "one":
        k = len(per[0])
        return f"5/one/{t}/spec{'0' if k == 0 else '1' if k == 1 else '2-4' if k <= 4 else '5up'}"
    flags = []
    if any(not s for s in per):
        flags.append("none")
    members = {}
    for i, specs in enumerate(per):
        for s in specs:
            members.setdefault(s, []).append(i)
    if any(len(v) > 1 for v in members.values()):
        flags.append("shared")
    if any(min(v, key=lambda i: (_full_key(best[i]), i)) != v[0] for v in members.values()):
        flags.append("late")
    return f"5/several/{t}" + "".join("+" + f for f in flags)


def situation(par, panel, prefilter, read):
    rrec = (read[0], O.revcomp(read[1]), read[2][::-1])
    return classify(panel, O.find_candidates(prefilter, par, panel, read, rrec))


def facets(label):
    """The census entries one label counts for."""
    base, *flags = label.split("+")
    return [base] + [f"5/several:{f}" for f in flags]


def census(par, panel, reads, ops=None):
    """(Counter over SITUATIONS + PROPERTIES, {read id: label}).  The properties are read from the oracle's records."""
    prefilter = O.make_prefilter(panel, par) if par.prefilter else None
    counts, labels = Counter(), {}
    for rec in reads:
        rrec = (rec[0], O.revcomp(rec[1]), rec[2][::-1])
        cands = O.find_candidates(prefilter, par, panel, rec, rrec)
        labels[rec[0]] = lab = classify(panel, cands)
        counts.update(facets(lab))
        if cands and par.dereplicate == "best":
            res = O.dereplicate(O.select_best(cands), panel)
            if len({id(e[0]) for e in res}) < len(res):
                counts["cand_twice"] += 1
    if ops is None:
        ops = O.process_sequences(reads, par, panel)[0]
    by_read = {}
    for op in ops:
        by_read.setdefault(op.seq_id, []).append(op)
    for rid, rops in by_read.items():
        if len(rops) > 1 and par.trim != "none":
            counts["multi_record"] += 1
        if any(is_fallback(op) for op in rops):
            counts["trim_empty"] += 1
        if "/untied" in labels[rid] and any(op.rtype == O.R_MULTI for op in rops):
            counts["multiple_untied"] += 1
    return counts, labels


def is_fallback(op):
    """A trim-to-empty fallback record (Q12): everything unknown, yet a primer was located."""
    return op.sample_id == "unknown" and op.pool == "unknown" and op.p1 == "unknown" and op.p2 == "unknown" and \
        bool(op.p1_loc or op.p2_loc)


def oracle_setup(pf, sf, **flags):
    """(panel, params) of the oracle for one flag set, the way parity_utils.Both builds them."""
    from parity_utils import make_args
    a = make_args(**flags)
    panel = O.load_panel(pf, sf)
    par = O.setup_params(panel, search_len=a.search_len, index_edit_distance=a.index_edit_distance,
                         primer_edit_distance=a.primer_edit_distance, preorient=not a.disable_preorient,
                         prefilter=not a.disable_prefilter, trim=a.trim, dereplicate=a.dereplicate,
                         min_length=a.min_length, max_length=a.max_length)
    return panel, par
