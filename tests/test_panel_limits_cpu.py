"""The envelope smx_panel_create admits, pinned on the host (no GPU needed): every limit of the panel compiler from both
sides, the launch plan of every panel tests/test_panel_limits_gpu.py runs, and the census that keeps those runs honest.

Limits: for each dimension the largest admitted panel compiles to a plan whose LDS stays within the pool in every mode, the
smallest refused one raises SmxError(ERR_UNSUPPORTED) with the limit in its text -- through compiled_panel, the way a user
meets it.  Two rows cannot be reached through a sheet and are driven through the descriptor instead: barcode_len_max +
k_index <= 200 (a barcode has at most 32 nt and k_index < its length, so a sheet reaches 63) and prefilter_min_len 1.
Plans: limits_utils.*_want reads R, MBW, G, CAPH, bs_ok, use64, pre_ok and the variant rows from CompiledPanel.plan().
Census: oracle only, in the style of test_scorer_cases_cpu.py and test_primer_cases_cpu.py."""
import ctypes as C
import os
import random
import re

import pytest

import limits_utils as LU
from scorer_utils import oracle_setup


def refused(pf, sf, text, **flags):
    from specimux_amd import _lib
    with pytest.raises(_lib.SmxError) as ei:
        LU.compile_panel(pf, sf, **flags)
    assert ei.value.code == _lib.ERR_UNSUPPORTED and re.search(text, str(ei.value)), str(ei.value)
    return str(ei.value)


def admitted(pf, sf, **flags):
    _both, cp = LU.compile_panel(pf, sf, **flags)
    plan = cp.plan()
    LU.assert_fits(plan, os.path.basename(os.path.dirname(pf)))
    return cp, plan


def write(sheet, tmp_path):
    return sheet.write(os.fspath(tmp_path / sheet.name))


# ------------------------------------------------------------------ every limit
def test_limit_distinct_primers(tmp_path):
    sheet = LU.many_primers_sheet(32)
    cp, plan = admitted(*write(sheet, tmp_path), **LU.A_BASE)
    assert cp.hits_per_read == 128 and (int(cp._keep["spec_p1mask"].max()) | int(cp._keep["spec_p2mask"].max())) >> 63 == 1
    sheet.primers.append(("FX", "P00", "forward", "ACGGATTACCAGTCAGGTCA"))
    sheet.rows.append(("P00_FX", "P00", sheet.fwd[1], "FX", sheet.rev[1], "R00"))
    sheet.name = "pools32_plus1"
    refused(*write(sheet, tmp_path), r"more than 64 distinct primers \(65\)", **LU.A_BASE)
    refused(*write(LU.many_primers_sheet(33), tmp_path), r"more than 64 distinct primers \(66\)", **LU.A_BASE)


def test_limit_primer_pairs(tmp_path):
    rng = random.Random(5)
    seqs = LU.distinct_seqs(rng, 31, 20, 9)

    def sheet(n_rev_y):   # wildcard rows pair every forward primer of a pool with every reverse primer of it: 12 x 10 + 1 x n
        primers = [(f"F{i}", "X", "forward", seqs[i]) for i in range(12)] + [(f"R{i}", "X", "reverse", seqs[12 + i]) for i in range(10)]
        primers += [("FY", "Y", "forward", seqs[22])] + [(f"RY{i}", "Y", "reverse", seqs[23 + i]) for i in range(n_rev_y)]
        rows = [(f"{pool}{j}", pool, b1, "*", b2, "*") for pool in "XY"
                for j, (b1, b2) in enumerate([("ACGTACGTACGTA", "TTGCAAGGTCAAC"), ("GGATCCAATTGCA", "CATGCATTTGGAC")])]
        return LU.Sheet(f"pairs{120 + n_rev_y}", primers, rows, [], [])
    cp, _plan = admitted(*write(sheet(7), tmp_path))
    assert len(cp.pairs) == 127
    refused(*write(sheet(8), tmp_path), r"more than 127 primer pairs \(128\)")


def _barcodes(n, avoid=(), seed=9, length=13):
    rng = random.Random(seed)
    out, seen = [], set(avoid)
    while len(out) < n:
        c = LU.rand_seq(rng, length)
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def _barcode_sheet(name, fwd, rev):
    """One primer pair; forward barcode i with reverse barcode i mod len(rev)."""
    rows = [(f"s{i}", "X", f, "F", rev[i % len(rev)], "R") for i, f in enumerate(fwd)]
    return LU.Sheet(name, [("F", "X", "forward", LU.ITS1F), ("R", "X", "reverse", LU.ITS4)], rows, fwd, rev)


def test_limit_barcodes_on_one_primer_and_the_lds_pool(tmp_path):
    """1024 barcodes on one primer are admitted while the panel has at most 1024 distinct barcodes (the reverse barcodes
    here are two of the forward strings); one distinct barcode more doubles the per-barcode kernel's Peq table, its tile of one
    read no longer fits the pool, and the panel is refused as a whole, with both numbers.  The parent accepted these."""
    flags = dict(index_edit_distance=3, disable_prefilter=True)
    two = ["CTACTTAGAATTA", "TACACCGAATGCT"]
    fwd = _barcodes(1025, avoid=two)
    cp, plan = admitted(*write(_barcode_sheet("maxB1024_NB1024", fwd[:1024], fwd[:2]), tmp_path), **flags)
    assert cp.max_barcodes == 1024 and len(cp.barcodes) == 1024 and plan.slots.MBW == 32 and plan.slots.G == 1024
    cp, plan = admitted(*write(_barcode_sheet("maxB1022_NB1024", fwd[:1022], two), tmp_path), **flags)
    assert cp.max_barcodes == 1022 and len(cp.barcodes) == 1024
    for n, trim in ((1023, "barcodes"), (1024, "barcodes"), (1024, "tails")):
        msg = refused(*write(_barcode_sheet(f"maxB{n}_NB{n + 2}", fwd[:n], two), tmp_path),
                      r"slots tiles of 1 read.* do not fit the LDS \(\d+ > 159744 bytes\)", trim=trim, **flags)
        need = int(re.search(r"\((\d+) > 159744 bytes\)", msg).group(1))
        assert 159744 < need <= 160 * 1024, "above the pool, and below the limit the parent compared with"
    refused(*write(_barcode_sheet("maxB1025", fwd, two[:1]), tmp_path), r"more than 1024 barcodes on one primer \(1025\)", **flags)


def _dealt_sheet(n_pools, bcs):
    """n_pools pools of one forward and one reverse primer; the barcodes dealt round robin over the 2 n_pools primers."""
    seqs = LU.distinct_seqs(random.Random(3), 2 * n_pools, 20, 9)
    lists = [bcs[p::2 * n_pools] for p in range(2 * n_pools)]
    primers, rows = [], []
    for i in range(n_pools):
        primers += [(f"F{i}", f"P{i}", "forward", seqs[2 * i]), (f"R{i}", f"P{i}", "reverse", seqs[2 * i + 1])]
        f, r = lists[2 * i], lists[2 * i + 1]
        rows += [(f"s{i}_{j}", f"P{i}", b, f"F{i}", r[j % len(r)], f"R{i}") for j, b in enumerate(f)]
    return LU.Sheet(f"dealt{n_pools}_{len(bcs)}", primers, rows, [], [])


def test_limit_distinct_barcodes(tmp_path):
    """The per-barcode kernel's Peq table takes 64 bytes per distinct barcode, the count rounded up to a power of two.  Up
    to 1024 barcodes that is 64 KiB and the other limits decide.  From 1025 to 2048 it is 128 KiB: most panels are then
    refused by the LDS rule (the one-pair panel below; 1025 barcodes in test_limit_barcodes_on_one_primer_and_the_lds_pool),
    a few shapes still fit -- six primers of about 216 barcodes each hold 1297 under --trim tails, to the byte, and not 1298.  Above 2048 the
    table alone is larger than the pool: refused by count."""
    flags = dict(index_edit_distance=3, disable_prefilter=True)
    bcs = _barcodes(2049)
    for trim in ("barcodes", "tails"):
        cp, plan = admitted(*write(_dealt_sheet(3, bcs[:1297]), tmp_path), trim=trim, **flags)
        assert len(cp.barcodes) == 1297 and cp.hits_per_read == 12 and plan.slots.R == 1
    refused(*write(_dealt_sheet(3, bcs[:1298]), tmp_path), r"slots tiles of 1 read.*1298 barcodes.* do not fit the LDS \(\d+ > 159744 bytes\)",
            trim="tails", **flags)
    refused(*write(_barcode_sheet("NB2048", bcs[:1024], bcs[1024:2048]), tmp_path),
            r"2048 barcodes.* do not fit the LDS \(\d+ > 159744 bytes\)", **flags)
    refused(*write(_barcode_sheet("NB2049", bcs[:1025], bcs[1025:]), tmp_path), r"more than 2048 distinct barcodes \(2049\)", **flags)


def test_limit_barcode_length_and_index_distance(tmp_path):
    s32 = LU.long_barcodes_sheet(32)
    pf, sf = write(s32, tmp_path)
    cp, plan = admitted(pf, sf, index_edit_distance=31, disable_prefilter=True)       # k_index = length - 1
    assert cp.desc.barcode_len_max + cp.desc.k_index == 63 and not plan.bs_ok
    refused(pf, sf, r"index edit distance 32 >= barcode length 32", index_edit_distance=32, disable_prefilter=True)   # k_index = length
    refused(pf, sf, r"index edit distance 33 outside 0\.\.32", index_edit_distance=33, disable_prefilter=True)
    refused(pf, sf, r"prefilter min length 1 < 2", index_edit_distance=31)             # the prefilter's L - k = 1
    admitted(pf, sf, index_edit_distance=30)                                           # ... and 2
    s33 = LU.one_pair("bc33", [b + "A" for b in s32.fwd], s32.rev)
    refused(*write(s33, tmp_path), r"barcode \d has length 33 \(supported 1\.\.32\)", index_edit_distance=8, disable_prefilter=True)
    one = LU.one_pair("bc1", ["A", "C"], ["G", "T"])
    cp, _plan = admitted(*write(one, tmp_path), index_edit_distance=0, disable_prefilter=True)
    assert cp.desc.barcode_len_max == 1


def test_limit_barcode_length_plus_k_through_the_descriptor(tmp_path):
    """barcode_len_max + k_index <= 200 and prefilter_min_len >= 2 guard descriptors no sheet can produce."""
    from specimux_amd import _lib
    lib = _lib.load()
    cp, _plan = admitted(*write(LU.long_barcodes_sheet(32), tmp_path), index_edit_distance=31, disable_prefilter=True)

    def create(**fields):
        d = _lib.PanelDesc.from_buffer_copy(cp.desc)
        for k, v in fields.items():
            setattr(d, k, v)
        h = C.c_void_p()
        rc = lib.smx_panel_create(C.byref(d), C.byref(h))
        msg = lib.smx_last_error().decode() if rc else ""
        if rc == 0:
            lib.smx_panel_destroy(h)
        return rc, msg
    assert create(barcode_len_max=169)[0] == _lib.OK                                        # 169 + 31 = 200
    assert create(barcode_len_max=170) == (_lib.ERR_UNSUPPORTED, "barcode length + k too large")
    assert create(prefilter_min_len=2)[0] == _lib.OK
    rc, msg = create(prefilter_min_len=1)
    assert rc == _lib.ERR_UNSUPPORTED and "prefilter min length 1 < 2" in msg


def test_limit_primer_length(tmp_path):
    """test_host_cpu.py::test_panel_limits_fail_loudly holds the 68-nt case; here the two sides of the limit itself."""
    cp, plan = admitted(*write(LU.primer_edge_sheet(64, "13k3"), tmp_path), index_edit_distance=3)
    assert plan.use64 and max(len(p.primer) for p in cp.primers) == 64
    s65 = LU.one_pair("m65", LU.primer_edge_sheet(64, "13k3").fwd, LU.primer_edge_sheet(64, "13k3").rev, fwd_primer=LU.LONG_PRIMER[:65])
    refused(*write(s65, tmp_path), r"primer 0 has length 65 \(supported 1\.\.64\)", index_edit_distance=3)
    s1 = LU.one_pair("m1", s65.fwd, s65.rev, fwd_primer="A")
    cp, _plan = admitted(*write(s1, tmp_path), index_edit_distance=3)                  # length 1: k = 0 < length
    assert min(len(p.primer) for p in cp.primers) == 1


def test_limit_search_len(tmp_path):
    pf, sf = write(LU.odd_window_sheet(), tmp_path)
    for S in (1, 256):
        _cp, plan = admitted(pf, sf, search_len=S, **LU.E_BASE)
        assert plan.pre_ok == (S == 256)
    refused(pf, sf, r"search_len 0 outside 1\.\.256", search_len=0, **LU.E_BASE)
    refused(pf, sf, r"search_len 257 outside 1\.\.256", search_len=257, **LU.E_BASE)


def test_limit_tile_size(tmp_path, monkeypatch):
    """The tile size is the planner's: 64 reads where they fit, halved until the tile fits its LDS budget, never below one
    read.  SMX_TILE_R reaches 1..64 (values outside are clamped); a tile of one read that still does not fit is the LDS refusal."""
    pf, sf = write(LU.primer_edge_sheet(31, "13k3"), tmp_path)
    for env, want in ((None, 64), ("1", 1), ("0", 1), ("64", 64), ("1000", 64)):
        if env is not None:
            monkeypatch.setenv("SMX_TILE_R", env)
        _cp, plan = admitted(pf, sf, index_edit_distance=3)
        assert (plan.lean.R, plan.slots.R) == (want, want)


# ------------------------------------------------------------------ the plan is what the corner needs
@pytest.mark.parametrize("n_pools", LU.A_POOLS)
def test_plan_many_primers(tmp_path_factory, monkeypatch, n_pools):
    pf, sf = LU.written(LU.memo(LU.many_primers_sheet, n_pools), tmp_path_factory)
    for env in LU.A_ENVS:
        with monkeypatch.context() as mp:
            for k, v in LU.a_env(env, n_pools).items():
                mp.setenv(k, v)
            for fl in LU.FLAG_SETS:
                _both, cp = LU.compile_panel(pf, sf, **LU.A_BASE, **fl)
                plan = cp.plan()
                LU.assert_fits(plan, f"{n_pools} pools {env} {fl}")
                LU.a_want(plan, cp, n_pools, env, fl)
    assert n_pools != 16 or cp.hits_per_read == 64      # the last panel whose alignments fit one 64-bit mask per read


@pytest.mark.parametrize("maxB", sorted(LU.B_SIZES))
def test_plan_many_barcodes(tmp_path_factory, maxB):
    sheet, _info = LU.memo(LU.many_barcodes_sheet, maxB)
    pf, sf = LU.written(sheet, tmp_path_factory)
    for k in LU.B_KS:
        for fl in LU.FLAG_SETS:
            _both, cp = LU.compile_panel(pf, sf, **LU.b_base(k), **fl)
            plan = cp.plan()
            LU.assert_fits(plan, f"maxB {maxB} k {k} {fl}")
            LU.b_want(plan, cp, maxB, k, fl)


@pytest.mark.parametrize("L,k,caps", LU.C_CELLS)
def test_plan_long_barcodes(tmp_path_factory, monkeypatch, L, k, caps):
    pf, sf = LU.written(LU.memo(LU.long_barcodes_sheet, L), tmp_path_factory)
    if caps:
        monkeypatch.setenv("SMX_TEST_CAPS", caps)
    for fl in LU.FLAG_SETS:
        _both, cp = LU.compile_panel(pf, sf, **LU.c_base(k), **fl)
        plan = cp.plan()
        LU.assert_fits(plan, f"{L} nt k {k} {fl}")
        LU.c_want(plan, cp, L, k, caps)


@pytest.mark.parametrize("m", LU.D_LENGTHS)
def test_plan_primer_word_edges(tmp_path_factory, m):
    rows = set()
    for variant, base in LU.D_PANELS:
        pf, sf = LU.written(LU.memo(LU.primer_edge_sheet, m, variant), tmp_path_factory)
        for flags in LU.FLAG_SETS:
            fl = dict(base, **flags)
            for S in LU.D_WINDOWS:
                _both, cp = LU.compile_panel(pf, sf, search_len=S, **fl)
                plan = cp.plan()
                LU.assert_fits(plan, f"{m} nt {variant} S {S} {fl}")
                LU.d_want(plan, m, variant, fl)
                rows.add(plan.lean.variant)
    if m > 32:
        assert rows == {(64, b, 0, 0) for b in range(4)}, rows


def test_plan_odd_windows(tmp_path_factory):
    from specimux_amd import synth
    pf, sf = LU.written(LU.memo(LU.odd_window_sheet), tmp_path_factory)
    for S in (1, 2) + LU.E_WINDOWS:
        for fl in LU.FLAG_SETS:
            plan = LU.compile_panel(pf, sf, search_len=S, **LU.E_BASE, **fl)[1].plan()
            LU.assert_fits(plan, f"S {S} {fl}")
            LU.e_want(plan, S)
    pf, sf = synth.panel_c2().write(os.fspath(tmp_path_factory.mktemp("c2")))
    LU.e_want(LU.compile_panel(pf, sf, search_len=255)[1].plan(), 255)


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_plan_small_tiles(tmp_path_factory, monkeypatch, name):
    from specimux_amd import synth
    pf, sf = getattr(synth, "panel_" + name)().write(os.fspath(tmp_path_factory.mktemp(name)))
    for r in LU.F_TILES:
        for env in LU.f_envs(r):
            with monkeypatch.context() as mp:
                for k, v in env.items():
                    mp.setenv(k, v)
                for fl in LU.FLAG_SETS:
                    _both, cp = LU.compile_panel(pf, sf, **fl)
                    plan = cp.plan()
                    LU.assert_fits(plan, f"{name} {env} {fl}")
                    LU.f_want(plan, r, env, len(cp.primers))


# ------------------------------------------------------------------ the census (oracle only)
@pytest.mark.parametrize("n_pools", LU.A_POOLS)
def test_census_many_primers(tmp_path_factory, n_pools):
    sheet = LU.memo(LU.many_primers_sheet, n_pools)
    pf, sf = LU.written(sheet, tmp_path_factory)
    reads, fam = LU.memo(LU.many_primers_reads, sheet, n_pools)
    assert 200 <= len(reads) <= 320
    panel, par = oracle_setup(pf, sf, **LU.A_BASE)
    c = LU.many_primers_census(sheet, par, panel, reads, fam)
    print(n_pools, "pools:", len(reads), "reads;", {k: v for k, v in c.items() if not isinstance(k, tuple)},
          "fewest per pool and orientation", min(c[("pool", i, o)] for i in range(n_pools) for o in "fr"))
    for i in range(n_pools):
        for o in "fr":
            assert c[("pool", i, o)] >= LU.MIN_POOL, (i, o, c[("pool", i, o)])
    for k in ("n_read", "short", "no_primer", "cross", "cross_pair"):
        assert c[k] >= LU.MIN_READS, (k, c[k])


@pytest.mark.parametrize("maxB", sorted(LU.B_SIZES))
@pytest.mark.parametrize("k", LU.B_KS)
def test_census_many_barcodes(tmp_path_factory, maxB, k):
    sheet, _info = LU.memo(LU.many_barcodes_sheet, maxB)
    pf, sf = LU.written(sheet, tmp_path_factory)
    reads, fam = LU.memo(LU.b_reads, maxB, k)
    assert 200 <= len(reads) <= 320
    panel, par = oracle_setup(pf, sf, **LU.b_base(k))
    c = LU.barcode_census(sheet, par, panel, reads, fam)
    print(f"maxB {maxB} k {k}: {len(reads)} reads;", dict(c))
    want = [("idx", i) for i in (0, 31, 32, 63, 64, maxB - 2, maxB - 1)] + [("tie", 2), ("tie", 3), ("dist", k), ("dist", k + 1), "none"]
    for f in want:
        assert c[f] >= LU.MIN_READS, (f, c[f])


@pytest.mark.parametrize("L,k", sorted({(L, k) for L, k, _c in LU.C_CELLS}))
def test_census_long_barcodes(tmp_path_factory, L, k):
    sheet = LU.memo(LU.long_barcodes_sheet, L)
    pf, sf = LU.written(sheet, tmp_path_factory)
    panel, par = oracle_setup(pf, sf, **LU.c_base(k))
    reads, fam = LU.memo(LU.c_reads, L, k, pf, sf)
    c = LU.long_barcodes_census(sheet, par, panel, reads, fam)
    print(f"{L} nt k {k}: {len(reads)} reads;", dict(c))
    for kind in ("sub", "indel", "cut"):
        for d in ("k-1", "k", "k+1"):
            # what cannot be built (long_barcodes_reads): a 32-nt barcode at distance 32, and at k = 31 anything but a cut read
            cannot = (d == "k+1" and k + 1 >= L) or (k == L - 1 and kind != "cut")
            assert (c[(kind, d)] == 0) if cannot else (c[(kind, d)] >= LU.MIN_READS), (kind, d, c[(kind, d)])


@pytest.mark.parametrize("m", LU.D_LENGTHS)
@pytest.mark.parametrize("S", LU.D_WINDOWS)
@pytest.mark.parametrize("variant,base", LU.D_PANELS, ids=[v for v, _b in LU.D_PANELS])
def test_census_primer_word_edges(tmp_path_factory, variant, base, m, S):
    sheet = LU.memo(LU.primer_edge_sheet, m, variant)
    pf, sf = LU.written(sheet, tmp_path_factory)
    reads, fam = LU.memo(LU.primer_edge_reads, sheet, m, S)
    assert 200 <= len(reads) <= 320
    panel, par = oracle_setup(pf, sf, search_len=S, **base)
    assert par.max_dist_primers[LU.LONG_PRIMER[:m]] == m // 3
    c = LU.primer_edge_census(par, panel, reads, fam)
    print(f"{m} nt {variant} S {S}: {len(reads)} reads;", dict(c))
    for label in ("d0", "first", "last", "firstlast", "dk", "dk1", "dk_indel", "noprimer"):
        assert c[label] >= LU.MIN_READS, (label, c[label])


@pytest.mark.parametrize("S", (1, 2) + LU.E_WINDOWS)
def test_census_odd_windows(tmp_path_factory, S):
    from oracle import specimux_oracle as O
    sheet = LU.memo(LU.odd_window_sheet)
    pf, sf = LU.written(sheet, tmp_path_factory)
    reads = LU.memo(LU.odd_window_reads, sheet)
    assert 200 <= len(reads) <= 320
    panel, par = oracle_setup(pf, sf, search_len=S, **LU.E_BASE)
    ops = O.process_sequences(reads, par, panel)[0]
    full = sum(op.rtype in LU.FULL for op in ops)
    unknown = sum(op.rtype == O.R_UNKNOWN for op in ops)
    print(f"S {S}: {len(reads)} reads, {full} full records, {unknown} unknown")
    if S <= 2:      # nothing fits such a window: every read is unknown, and the kernel must say the same
        assert unknown == len(ops) == len(reads)
    else:
        assert full >= LU.MIN_READS and unknown >= LU.MIN_READS
