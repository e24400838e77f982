"""Panels at the edges of what smx_panel_create admits, constructed reads for them and a census -- shared by
tests/test_panel_limits_cpu.py (limits, plans and the census, no GPU) and tests/test_panel_limits_gpu.py (the kernel against the
oracle).  Plain Python; what a read "is" is decided by the oracle alone.

Per section (a many primers, b many barcodes on one primer, c long barcodes and large k, d primer word edges, e odd
windows, f small tiles): a sheet builder, a read builder that also says which family a read belongs to, a census that counts
the reads of each family that are in the intended situation under the oracle (at least MIN_READS; MIN_POOL per pool and
orientation), and `*_want`, which asserts from CompiledPanel.plan() the property of the launch plan the case exists for --
a planner change that moves the corner fails on the host and says so."""
import os
import random
from collections import Counter

from oracle import specimux_oracle as O

MIN_READS, MIN_POOL = 8, 4
HEADER = "SampleID\tPrimerPool\tFwIndex\tFwPrimer\tRvIndex\tRvPrimer\n"
FLAG_SETS = [dict(), dict(trim="tails"), dict(trim="primers"), dict(dereplicate="none")]
ITS1F, ITS4 = "CTTGGTCATTTAGAGGAAGTAA", "TCCTCCGCTTATTGATATGC"
FULL = (O.R_FULL, O.R_DEREP)


def flag_id(f):
    return ",".join(f"{k}={v}" for k, v in f.items()) or "default"


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def sub(s, *pos):
    s = list(s)
    for p in pos:
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
    return "".join(s)


def indels(s, d, rng):
    """d edits, deletions and insertions in turn, at inner positions."""
    s = list(s)
    for i in range(d):
        p = rng.randrange(1, max(2, len(s) - 1))
        if i % 2 == 0 and len(s) > 2:
            del s[p]
        else:
            s.insert(p, rng.choice("ACGT"))
    return "".join(s)


def distinct_seqs(rng, n, length, min_dist):
    """n sequences at pairwise edit distance >= min_dist, their reverse complements included (primers of one panel)."""
    from oracle import edlib_semantics as E
    out = []
    while len(out) < n:
        c = rand_seq(rng, length)
        if all(E.align(c, x, E.NW, -1, iupac=False)["editDistance"] >= min_dist and
               E.align(O.revcomp(c), x, E.NW, -1, iupac=False)["editDistance"] >= min_dist for x in out):
            out.append(c)
    return out


class Sheet:
    """A primer file and a specimen sheet.  primers: (name, pools, position, sequence); rows: the sheet's six columns."""

    def __init__(self, name, primers, rows, fwd, rev):
        self.name, self.primers, self.rows, self.fwd, self.rev = name, primers, rows, fwd, rev   # fwd / rev: barcode lists

    def write(self, d):
        os.makedirs(d, exist_ok=True)
        pf, sf = os.path.join(d, "primers.fasta"), os.path.join(d, "specimens.txt")
        with open(pf, "w") as fh:
            for name, pools, pos, seq in self.primers:
                fh.write(f">{name} pool={pools} position={pos}\n{seq}\n")
        with open(sf, "w") as fh:
            fh.write(HEADER)
            for row in self.rows:
                fh.write("\t".join(row) + "\n")
        return pf, sf

    def primer(self, name):
        return next(s for n, _p, _d, s in self.primers if n == name)


def one_pair(name, fwd_bcs, rev_bcs, fwd_primer=ITS1F, rev_primer=ITS4):
    rows = [(f"s{i:04d}_{j}", "X", f, "F", r, "R") for i, f in enumerate(fwd_bcs) for j, r in enumerate(rev_bcs)]
    return Sheet(name, [("F", "X", "forward", fwd_primer), ("R", "X", "reverse", rev_primer)], rows, fwd_bcs, rev_bcs)


def structure(fb, fp, rb, rp, ins, head="TTTT", tail="GGGG"):
    left = head + fb + fp if fp else head
    right = O.revcomp(rp) + O.revcomp(rb) + tail if rp else tail
    return left + ins + right


def with_quals(reads, seed):
    rng = random.Random(seed)
    assert len({rid for rid, _s in reads}) == len(reads)
    return [(rid, s, "".join(chr(33 + rng.randrange(3, 41)) for _ in s)) for rid, s in reads]


def flagged_reads(fb, fp, rb, rp, rng, tag):
    """A short read, a read with an N in its head window and a lower-case read: the reads the prescan does not take."""
    good = structure(fb, fp, rb, rp, rand_seq(rng, 200))
    return [(f"{tag}_short", good[:45]), (f"{tag}_n", good[:50] + "N" + good[51:]), (f"{tag}_lower", good.lower())]


# ------------------------------------------------------------------ a. many primers
def many_primers_sheet(n_pools):
    """n_pools pools of one forward and one reverse 20-nt primer, a 4 x 3 barcode grid in each; pool i also pairs its forward
    primer with the reverse primer of pool i + 1 (one specimen), so that the panel has 2 n_pools primer pairs."""
    from specimux_amd import synth
    rng = random.Random(1000 + n_pools)
    seqs = distinct_seqs(rng, 2 * n_pools, 20, 9)
    F, R = synth.make_barcodes(4, 3, 13, 6, seed=41)
    pool = [f"P{i:02d}" for i in range(n_pools)]
    primers, rows = [], []
    for i in range(n_pools):
        primers.append((f"F{i:02d}", pool[i], "forward", seqs[2 * i]))
        primers.append((f"R{i:02d}", f"{pool[i]},{pool[(i - 1) % n_pools]}", "reverse", seqs[2 * i + 1]))
    for i in range(n_pools):
        rows += [(f"{pool[i]}_F{a}_R{b}", pool[i], F[a], f"F{i:02d}", R[b], f"R{i:02d}") for a in range(4) for b in range(3)]
        rows.append((f"{pool[i]}_X", pool[i], F[0], f"F{i:02d}", R[1], f"R{(i + 1) % n_pools:02d}"))
    return Sheet(f"pools{n_pools}", primers, rows, F, R)


def many_primers_reads(sheet, n_pools):
    rng = random.Random(2000 + n_pools)
    F, R = sheet.fwd, sheet.rev
    fp = [sheet.primer(f"F{i:02d}") for i in range(n_pools)]
    rp = [sheet.primer(f"R{i:02d}") for i in range(n_pools)]
    per = 4 if n_pools > 20 else 6
    out, fam = [], {}

    def add(rid, s, family, o="f"):
        out.append((rid, s if o == "f" else O.revcomp(s)))
        fam[rid] = family

    for i in range(n_pools):
        for o in "fr":
            for r in range(per):
                a, b = (r + i) % 4, (r + 2 * i) % 3
                fb, p = F[a], fp[i]
                if r == 1:
                    fb = sub(fb, 6)
                elif r == 2:
                    p = sub(p, 9)
                elif r == 3:
                    p = p[:7] + "A" + p[7:]
                add(f"pool{i:02d}_{o}{r}", structure(fb, p, R[b], rp[i], rand_seq(rng, rng.randrange(120, 300))), ("pool", i, o, f"P{i:02d}_F{a}_R{b}"), o)
    for j in range(10):
        i = (n_pools - 1, 0, n_pools // 2)[j % 3]   # the last pool first
        s = structure(F[j % 4], fp[i], R[j % 3], rp[i], rand_seq(rng, 220))
        add(f"n_{j}", s[:48 + j] + "N" + s[49 + j:], ("n_read", i), "fr"[j % 2])
    for j in range(12):
        i = (n_pools - 1, 1, n_pools // 2)[j % 3]
        # (a read of L < search_len is searched in its last search_len - L bases only: the reference's negative slice start)
        add(f"short_{j}", ("TT" + F[j % 4] + fp[i] + rand_seq(rng, 60))[:36 + j], ("short", i), "fr"[j % 2])
    for j in range(10):
        # (random text will not do: among 64 random 20-nt primers one is within 6 edits of some stretch of most reads)
        add(f"noprimer_{j}", ("A" * (7 + j) + "CAAT"[j % 4]) * (12 + j), ("no_primer",))
    for j in range(10):
        i = (n_pools - 1 - j) % n_pools
        add(f"cross_{j}", structure(F[j % 4], fp[i], R[j % 3], rp[(i + 5) % n_pools], rand_seq(rng, 200)), ("cross", i), "fr"[j % 2])
    for j in range(10):
        i = (n_pools - 1 - j) % n_pools
        add(f"crosspair_{j}", structure(F[0], fp[i], R[1], rp[(i + 1) % n_pools], rand_seq(rng, 200)), ("cross_pair", i), "fr"[j % 2])
    rng.shuffle(out)   # the 32 reads with an N or shorter than the window end up in nearly every tile of 16 to 48 reads
    # Eight more reads with an N, side by side at the front.  A read with an N takes a record for each of its 2 NP >= 64
    # alignments, a compact tile has 8 reads or more and 256 records at the most: the first tile goes to the redo launch
    # whatever the planner makes of the rest.
    front = []
    for j in range(8):
        i = (n_pools - 1, 0)[j % 2]
        s = structure(F[j % 4], fp[i], R[j % 3], rp[i], rand_seq(rng, 220))
        s = s[:50 + j] + "N" + s[51 + j:]
        front.append((f"nfront_{j}", s if j % 2 == 0 else O.revcomp(s)))
        fam[f"nfront_{j}"] = ("n_read", i)
    out[:0] = front
    return with_quals(out, 3000 + n_pools), fam


def many_primers_census(sheet, par, panel, reads, fam, S=80):
    """Counter over ("pool", i, o), "n_read", "short", "no_primer", "cross", "cross_pair": reads of each family that are what
    the family is for under the oracle."""
    by = {}
    for op in O.process_sequences(reads, par, panel)[0]:
        by.setdefault(op.seq_id, []).append(op)
    names = [n for n, _p, _d, _s in sheet.primers]
    c = Counter()
    for rid, s, _q in reads:
        f, ops = fam[rid], by[rid]
        full = [op for op in ops if op.rtype in FULL]
        if f[0] == "pool":
            c[f[:3]] += any(op.sample_id == f[3] and op.pool == f[3][:3] for op in full)
        elif f[0] == "n_read":
            c["n_read"] += len(full) == 1 and "N" in s[:S] + s[-S:]
        elif f[0] == "short":
            t = O.hit_table(par, panel, (rid, s, _q))
            c["short"] += len(s) < S and max(t[(f"F{f[1]:02d}", e)]["pdist"] for e in "AB") >= 0
        elif f[0] == "no_primer":
            c["no_primer"] += len(ops) == 1 and ops[0].rtype == O.R_UNKNOWN and ops[0].p1 == "unknown" and ops[0].p2 == "unknown"
        elif f[0] == "cross":     # both primers are found, yet the sheet pairs them nowhere: no full match
            t = O.hit_table(par, panel, (rid, s, _q))
            found = {n for n in names if t[(n, "A")]["pdist"] >= 0 or t[(n, "B")]["pdist"] >= 0}
            c["cross"] += not full and {f"F{f[1]:02d}", f"R{(f[1] + 5) % (len(names) // 2):02d}"} <= found
        elif f[0] == "cross_pair":
            c["cross_pair"] += len(full) == 1 and full[0].sample_id == f"P{f[1]:02d}_X"
    return c


# ------------------------------------------------------------------ b. many barcodes on one primer
def many_barcodes_sheet(maxB):
    """One primer pair, maxB forward and 2 reverse 13-nt barcodes.  Planted among the random forward barcodes, in three
    different tie-mask words: X, X with two substitutions (twice) -- a text between them is at distance 2 from two or three --
    and Y with one substitution at one position (three letters) -- a fourth letter there is at distance 1 from all three."""
    rng = random.Random(5000 + maxB)
    seen, fwd = set(), []
    while len(fwd) < maxB:
        c = rand_seq(rng, 13)
        if c not in seen:
            seen.add(c)
            fwd.append(c)
    X, Y = "ACCGTTGACAGTC", "GGATCTACGTTCA"
    last = (maxB - 1) // 32
    mid = 32 * (last // 2)
    plant = {5: X, mid + 6: sub(X, 2, 8), maxB - 1: sub(X, 5, 11),
             9: Y, mid + 11: Y[:6] + "C" + Y[7:], 32 * (last - 1) + 1: Y[:6] + "G" + Y[7:]}   # Y[6] = "A"
    assert last >= 4 and len({i // 32 for i in (5, mid + 6, maxB - 1)}) == 3 and len({i // 32 for i in (9, mid + 11, 32 * (last - 1) + 1)}) == 3
    for i, b in plant.items():
        assert b not in seen
        fwd[i] = b
    assert len(set(fwd)) == maxB
    rev = ["CTACTTAGAATTA", "TACACCGAATGCT"]
    return one_pair(f"maxB{maxB}", fwd, rev), {"X": X, "Y": Y, "plant": plant}


def many_barcodes_reads(sheet, info, maxB, k):
    rng = random.Random(6000 + maxB + k)
    fwd, rev = sheet.fwd, sheet.rev
    X, Y = info["X"], info["Y"]
    out, fam = [], {}

    def add(rid, fb, family, n=1, cut=0):
        for j in range(n):
            s = structure(fb, ITS1F, rev[j % 2], ITS4, rand_seq(rng, rng.randrange(100, 260)), head="TTTT"[:4 - cut] if cut < 4 else "")
            o = "fr"[j % 2]
            out.append((f"{rid}_{j}{o}", s if o == "f" else O.revcomp(s)))
            fam[f"{rid}_{j}{o}"] = family

    for idx in (0, 31, 32, 63, 64, maxB - 2, maxB - 1):
        add(f"idx{idx}", fwd[idx], ("idx", idx), 12)
    add("tie2a", sub(X, 2), ("tie", 2), 6)            # at 1 from X and from sub(X, 2, 8)
    add("tie2b", sub(X, 8), ("tie", 2), 6)
    add("tie3a", Y[:6] + "T" + Y[7:], ("tie", 3), 12)
    if k >= 2:
        add("tie3b", sub(sub(X, 2), 5), ("tie", 3), 6)    # at 2 from X, from sub(X, 2, 8) and from sub(X, 5, 11)
    for j in range(36):
        b = fwd[(37 * j + 11) % maxB]
        pos = list(range(13))
        rng.shuffle(pos)
        add(f"dk_{j}", sub(b, *pos[:k]), ("dist", k, b))
        add(f"dk1_{j}", sub(b, *pos[:k + 1]), ("dist", k + 1, b))
    for j in range(8):
        add(f"none_a{j}", "", ("none",), cut=4)          # the primer at the very start of the read: nothing to search
        add(f"none_b{j}", "", ("none",), cut=2)
        add(f"none_c{j}", rand_seq(rng, 13), ("none",))
    return with_quals(out, 7000 + maxB + k), fam


def barcode_census(sheet, par, panel, reads, fam, primer="F"):
    """Counter over ("idx", i), ("tie", n), ("dist", d), "none" from the oracle's hit table of the forward primer."""
    local = {b: i for i, b in enumerate(sheet.fwd)}
    c = Counter()
    for rec in reads:
        f = fam[rec[0]]
        t = O.hit_table(par, panel, rec)
        hs = [t[(primer, e)] for e in "AB" if t[(primer, e)]["pdist"] >= 0]
        if len(hs) != 1:
            continue
        d = {bc: v[0] for bc, v in hs[0]["barcodes"].items()}
        best = min(d.values()) if d else None
        tied = [b for b in d if d[b] == best]
        if f[0] == "idx":
            c[f] += tied == [sheet.fwd[f[1]]] and best == 0
        elif f[0] == "tie":
            c[f] += len(tied) == f[1] and len({local[b] // 32 for b in tied}) == f[1]
        elif f[0] == "dist":
            c[f[:2]] += (d.get(f[2]) == f[1]) if f[1] <= par.max_dist_index else (f[2] not in d)
        elif f[0] == "none":
            c["none"] += not d
    return c


# ------------------------------------------------------------------ c. long barcodes, large k
def long_barcodes_sheet(length):
    from specimux_amd import synth
    F, R = synth.make_barcodes(4, 3, length, 20 if length == 32 else 9, seed=77 + length)
    return one_pair(f"bc{length}", F, R)


def long_barcodes_reads(sheet, k, par, panel, per=20):
    """Texts in the forward barcode's place at k - 1, k and k + 1 edits from it, by substitutions and by indels, and barcodes cut
    short by the read's end.  A number of edits is not a distance (at k = 16 of 32 nt a random text is about that far away), so
    every text is kept or dropped by the distance the oracle finds for it, k + 1 under parameters that allow one edit more.
    What cannot be built: distance 32 from a 32-nt barcode is the empty target, which is never searched; and at k = 31 any
    text of three bases or more is nearer than 30 -- there the cut reads alone reach k - 1 and k."""
    import copy
    L = len(sheet.fwd[0])
    rng = random.Random(8000 + L + k)
    par1 = copy.copy(par)
    par1.max_dist_index = min(k + 1, L - 1)
    out, fam = [], {}

    def dist(rec, b, p):
        t = O.hit_table(p, panel, rec)
        hs = [t[("F", e)] for e in "AB" if t[("F", e)]["pdist"] >= 0]
        return {bc: v[0] for bc, v in hs[0]["barcodes"].items()}.get(b) if len(hs) == 1 else -1

    for kind in ("sub", "indel"):
        for d in (k - 1, k, k + 1):
            if d >= L or (k == L - 1 and d >= k - 1):
                continue
            n = 0
            for trial in range(2000):
                b, e = sheet.fwd[trial % 4], min(L, d + trial % 15) if kind == "sub" else d + trial % 40
                pos = list(range(L))
                rng.shuffle(pos)
                text = sub(b, *pos[:e]) if kind == "sub" else indels(b, e, rng)
                s = structure(text, ITS1F, sheet.rev[trial % 3], ITS4, rand_seq(rng, rng.randrange(100, 260)), head="TTGCA")
                rec = (f"{kind}{d}_{n}", s if trial % 2 == 0 else O.revcomp(s), "I" * len(s))
                if dist(rec, b, par1 if d > k else par) == d:
                    out.append(rec[:2])
                    fam[rec[0]] = (kind, d, b)
                    n += 1
                    if n == per:
                        break
    cuts = sorted({c for c in (1, 2, 3, k - 1, k, k + 1, L - 2, L - 1) if 1 <= c < L})
    for j in range(60):   # filler: the barcode itself, and a random text in its place (at a large k it is near every barcode)
        text = sheet.fwd[j % 4] if j % 2 else rand_seq(rng, L)
        s = structure(text, ITS1F, sheet.rev[j % 3], ITS4, rand_seq(rng, rng.randrange(100, 260)), head="TTGCA"[:j % 6])
        out.append((f"plain_{j}", s if j % 4 < 2 else O.revcomp(s)))
        fam[f"plain_{j}"] = ("plain", 0, text)
    for j in range(10):   # the read begins (ends, reverse complemented) inside the barcode: c of its bases are missing
        for c in cuts:
            b = sheet.fwd[(j + c) % 4]
            s = structure(b[c:], ITS1F, sheet.rev[j % 3], ITS4, rand_seq(rng, 180), head="")
            out.append((f"cut{c}_{j}", s if j % 2 == 0 else O.revcomp(s)))
            fam[f"cut{c}_{j}"] = ("cut", c, b)
    return with_quals(out, 9000 + L + k), fam


def long_barcodes_census(sheet, par, panel, reads, fam):
    """Counter over (kind, "k-1" | "k" | "k+1" [| "other" for the cut reads]): the true barcode is found at exactly that distance (k + 1: not found)."""
    k = par.max_dist_index
    c = Counter()
    for rec in reads:
        kind, d, b = fam[rec[0]]
        t = O.hit_table(par, panel, rec)
        hs = [t[("F", e)] for e in "AB" if t[("F", e)]["pdist"] >= 0]
        if len(hs) != 1 or kind == "plain":
            continue
        got = {bc: v[0] for bc, v in hs[0]["barcodes"].items()}.get(b)
        if kind == "cut":
            c[("cut", "k-1" if d == k - 1 else "k" if d == k else "k+1" if d == k + 1 else "other")] += got == d if d <= k else got is None
        else:
            c[(kind, {k - 1: "k-1", k: "k", k + 1: "k+1"}[d])] += (got == d) if d <= k else (got is None)
    return c


# ------------------------------------------------------------------ d. primer word edges
LONG_PRIMER = "GATCGGAAGAGCACACGTCTGAACTCCAGTCACTTAGGCATCTCGTATGCCGTCTTCTGCTTGAAACC"   # 68 nt, no repeat of 8 or more


def primer_edge_sheet(m, variant):
    """Forward primer of m nt.  variant: "13k3" (13-nt barcodes), "16k5" (16-nt) or "mixed" (12- and 13-nt barcodes)."""
    from specimux_amd import synth
    if variant == "16k5":
        F, R = synth.make_barcodes(4, 3, 16, 10, seed=5)
    else:
        F, R = synth.make_barcodes(4, 3, 13, 6, seed=6)
        if variant == "mixed":
            F = [F[0][:12], F[1], F[2][1:], F[3]]
    return one_pair(f"m{m}_{variant}", F, R, fwd_primer=LONG_PRIMER[:m])


def primer_edge_reads(sheet, m, S):
    p = LONG_PRIMER[:m]
    k = int(m / 3)                     # the reference's threshold for a primer of m unambiguous bases
    rng = random.Random(10000 + m + S)
    out, fam = [], {}
    texts = [("d0", p, 0), ("first", sub(p, 0), 1), ("last", sub(p, m - 1), 1), ("firstlast", sub(p, 0, m - 1), 2)]
    for j in range(40):    # (k substitutions are not always k edits: the second half of the loop adds to those two families only)
        o = "fr"[j % 2]
        pos = list(range(m))
        rng.shuffle(pos)
        cases = [("dk", sub(p, *pos[:k]), k), ("dk1", sub(p, *pos[:k + 1]), k + 1)]
        if j < 24:
            cases += texts + [("dk_indel", indels(p, k, rng), k)]
        for label, text, d in cases:
            head = "TTGA"[:min(j % 5, max(0, S - m - len(sheet.fwd[j % 4])))]    # (barcode and primer stay inside the window)
            s = structure(sheet.fwd[j % 4], text, sheet.rev[j % 3], ITS4, rand_seq(rng, rng.randrange(2 * S, 2 * S + 150)), head=head)
            rid = f"{label}_{j}{o}"
            out.append((rid, s if o == "f" else O.revcomp(s)))
            fam[rid] = (label, d)
    for j in range(12):
        out.append((f"noprimer_{j}", rand_seq(rng, 2 * S + 50)))
        fam[f"noprimer_{j}"] = ("noprimer", -1)
    return with_quals(out, 11000 + m + S), fam


def primer_edge_census(par, panel, reads, fam):
    """Counter over the labels: the forward primer is found at exactly the distance the text was built with (dk1, noprimer:
    not found)."""
    k = par.max_dist_primers[panel.by_name["F"].primer]
    c = Counter()
    for rec in reads:
        label, d = fam[rec[0]]
        t = O.hit_table(par, panel, rec)
        got = sorted(t[("F", e)]["pdist"] for e in "AB")[-1]
        if label in ("dk1", "noprimer"):
            c[label] += got == -1
        elif label == "dk_indel":
            c[label] += 0 < got <= k          # indels may cancel: within k, and not exact
        else:
            c[label] += got == d
    return c


# ------------------------------------------------------------------ e. odd windows
SHORT_F, SHORT_R = "GTCCAGTA", "CATGGTCAAG"     # 8 and 10 nt: thresholds 2 and 3


def odd_window_sheet():
    F = ["ACGTCA", "CTAGAG", "GGTTAC", "TACCGT"]
    R = ["AGGACT", "CTTCGA", "TGCATC"]
    return one_pair("short_primers", F, R, fwd_primer=SHORT_F, rev_primer=SHORT_R)


def odd_window_reads(sheet, n=220, seed=0):
    rng = random.Random(12000 + seed)
    out = []
    for j in range(n):
        fb, rb = sheet.fwd[j % 4], sheet.rev[j % 3]
        kind = j % 11
        if kind == 9:
            s = rand_seq(rng, rng.randrange(1, 60))                      # nothing, any length from 1
        elif kind == 10:
            s = structure(fb, SHORT_F, rb, SHORT_R, rand_seq(rng, 30), head="")[:rng.randrange(10, 40)]   # shorter than most windows
        else:
            fbt = sub(fb, j % 6) if kind == 3 else fb
            fpt = sub(SHORT_F, j % 8) if kind == 4 else SHORT_F
            head = "" if kind < 6 else "TTGAC"[:kind - 5]
            s = structure(fbt, fpt, rb, SHORT_R, rand_seq(rng, rng.randrange(0, 300)), head=head, tail=head)
            if kind == 5:
                s = s[:7] + "N" + s[8:]
        out.append((f"w{j}", s if j % 2 == 0 else O.revcomp(s)))
    return with_quals(out, 13000 + seed)


# ------------------------------------------------------------------ panels on disk, plans
def written(sheet, tmp_path_factory, _cache={}):
    """(primer file, specimen file) of a sheet, written once per session."""
    if sheet.name not in _cache:
        _cache[sheet.name] = sheet.write(os.fspath(tmp_path_factory.mktemp("lim_" + sheet.name)))
    return _cache[sheet.name]


def memo(fn, *args, _cache={}):
    """fn(*args), built once per session (sheets and reads are deterministic and are not modified)."""
    key = (fn.__name__,) + args
    if key not in _cache:
        _cache[key] = fn(*args)
    return _cache[key]


def b_reads(maxB, k):
    sheet, info = memo(many_barcodes_sheet, maxB)
    return many_barcodes_reads(sheet, info, maxB, k)


def c_reads(L, k, pf, sf):
    from scorer_utils import oracle_setup
    panel, par = oracle_setup(pf, sf, **c_base(k))
    return long_barcodes_reads(memo(long_barcodes_sheet, L), k, par, panel)


def compile_panel(pf, sf, **flags):
    """(Both, CompiledPanel) under the environment switches of the moment; needs no device."""
    from parity_utils import Both
    from specimux_amd.demultiplex import compiled_panel
    both = Both(pf, sf, **flags)
    return both, compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)


def assert_fits(plan, label=""):
    """Every mode the panel can launch stays within the LDS pool (checked on the host before anything is launched)."""
    for name in ("lean", "slots", "compact"):
        m = getattr(plan, name)
        assert m is None or 0 < m.lds <= plan.lds_pool, f"{label}: {name} tiles need {m.lds} bytes of LDS, the pool has {plan.lds_pool}"


def bsv_of(flags, bs_ok, k):
    """The barcode scan variant the lean kernel of a panel runs: 0 per barcode, 1 bit-sliced k <= 3, 2 k 4..7, 3 k <= 3 tails."""
    return 0 if not bs_ok else 2 if k > 3 else 3 if flags.get("trim") == "tails" else 1


# ---- a
A_POOLS = (16, 17, 32)
A_ENVS = ("default", "dense", "overflow", "no_prescan")
A_BASE = dict(index_edit_distance=3)


def a_env(env, n_pools):
    return {"default": {}, "dense": {"SMX_COMPACT": "0"}, "overflow": {"SMX_COMPACT_ITEMS": str(4 * n_pools)},
            "no_prescan": {"SMX_NO_PRESCAN": "1"}}[env]


def a_want(plan, cp, n_pools, env, flags):
    NP = 2 * n_pools
    assert cp.hits_per_read == 2 * NP and len(cp.pairs) == 2 * n_pools
    assert plan.lean.MBW == 1 and plan.bs_ok and not plan.use64
    bsv = bsv_of(flags, True, 3)
    assert plan.lean.R <= 16, "the dense tile of a many-primer panel has to shrink"
    if env == "no_prescan":
        assert not plan.pre_ok and plan.nitems == 0 and plan.lean.variant == (32, bsv, 0, 0)
    elif env == "dense":
        assert plan.pre_ok and plan.nitems == 0 and plan.compact is None and plan.lean.variant == (32, bsv, 0, 0)
    else:
        assert plan.pre_ok and plan.nitems == (2 * NP if env == "overflow" else 256)
        assert plan.compact.R > plan.lean.R and plan.compact.variant == (32, bsv, 1, 0) and plan.redo == (32, bsv, 2, 0)
    assert plan.slots.variant == (32, 0, 0, 0)


# ---- b
B_SIZES = {129: dict(MBW=5, G=256, slots_R=4), 512: dict(MBW=16, G=512, lean_R=8, slots_R=1),
           1000: dict(MBW=32, G=1024, lean_R=1, slots_R=1, CAPH=4)}
B_KS = (1, 3)


def b_base(k):
    return dict(index_edit_distance=k, disable_prefilter=True)


def b_want(plan, cp, maxB, k, flags):
    w = B_SIZES[maxB]
    assert cp.max_barcodes == maxB and cp.hits_per_read == 4
    for m in (plan.lean, plan.slots):
        assert (m.MBW, m.G) == (w["MBW"], w["G"])
    assert plan.slots.R == w["slots_R"] and plan.lean.R == w.get("lean_R", plan.lean.R)
    assert plan.bs_ok and plan.lean.variant == (32, bsv_of(flags, True, k), 0, 0) and plan.slots.variant == (32, 0, 0, 0)
    if "CAPH" in w:
        assert plan.lean.CAPH == plan.slots.CAPH == w["CAPH"]
    else:   # several barcode rounds per tile: fewer hits fit one round than a tile can hold
        assert plan.lean.CAPH < plan.lean.R * cp.hits_per_read


# ---- c
C_CELLS = [(32, 8, None), (32, 16, None), (32, 31, None), (32, 31, "3,80"), (17, 3, None), (17, 7, None)]   # length, k, SMX_TEST_CAPS


def c_base(k):
    return dict(index_edit_distance=k, disable_prefilter=True)


def c_want(plan, cp, L, k, caps):
    assert not plan.bs_ok and plan.lean.variant == (32, 0, 0, 0) and plan.slots.variant == (32, 0, 0, 0)
    assert cp.desc.barcode_len_max == L and cp.desc.k_index == k
    if caps:
        assert plan.lean.CAPH == int(caps.split(",")[0]) < plan.lean.R * cp.hits_per_read


# ---- d
D_LENGTHS = (31, 32, 33, 63, 64)
D_PANELS = [("13k3", dict(index_edit_distance=3)), ("16k5", dict(index_edit_distance=5)),     # each under every FLAG_SETS entry:
            ("mixed", dict(index_edit_distance=3, disable_prefilter=True))]                     # scan variants 1 and 3, 2, 0
D_WINDOWS = (80, 256)


def d_want(plan, m, variant, flags):
    bs = variant != "mixed"
    bsv = bsv_of(flags, bs, flags["index_edit_distance"])
    assert plan.use64 == (m > 32) and plan.pre_ok == (m <= 31) and plan.bs_ok == bs and plan.nitems == 0
    w = 64 if m > 32 else 32           # 32 nt: the top bit of the 32-bit word; 33: the first 64-bit word; 64: its top bit
    assert plan.lean.variant[:3] == (w, bsv, 0) and plan.slots.variant == (w, 0, 0, 0)
    assert m <= 31 or plan.lean.variant[3] == 0     # (only a launch behind the prescan can be a default-flags kernel)


# ---- e
E_WINDOWS = (15, 17, 31, 33, 255)
E_BASE = dict(index_edit_distance=1)


def e_want(plan, S):
    assert plan.pre_ok == (S % 16 == 0) and plan.nitems == 0 and plan.lean.R == (64 if S <= 128 else 32)


# ---- f
F_TILES = (1, 2, 4)


def f_envs(r):
    return [{"SMX_TILE_R": str(r)}, {"SMX_TILE_R": str(r), "SMX_COMPACT": "0"}, {"SMX_TILE_R": str(r), "SMX_PRESCAN_PLANES": "1"}]


def f_want(plan, r, env, n_primers):
    assert plan.lean.R == r and plan.slots.R <= r and plan.pre_ok
    assert plan.pre_tile == (n_primers <= 2 and "SMX_PRESCAN_PLANES" not in env)
    if "SMX_COMPACT" in env:
        assert plan.nitems == 0
    else:   # a shrunken dense tile turns compact tiles on wherever they keep more reads in flight
        assert plan.nitems == 256 and plan.compact.R > r and plan.redo[2] == 2
