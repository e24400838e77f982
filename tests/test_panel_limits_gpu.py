"""The demux kernel at the panel sizes smx_panel_create admits and no other test reaches (run on the MI355X box: `pytest -m
gpu`): odd windows (e), tiles of 1, 2 and 4 reads (f), primers at the 32- and 64-bit word edges (d), 32 to 64 distinct
primers (a), long barcodes at a large k (c), 129 to 1000 barcodes on one primer (b) -- in that order, the mild cases first
and the 1000-barcode panel last.  Records go through Both.assert_ops_equal, hit tables through assert_hits_equal with both
dumps, so the per-barcode ("slots") plan of every panel runs as well as the lean one; everything is compared bit for bit with
the CPU oracle.  Before anything is launched a case reads CompiledPanel.plan(): every mode fits the LDS pool, and the plan
is the one the case is about (limits_utils.*_want; tests/test_panel_limits_cpu.py holds the same checks and the census of
the reads, without a GPU)."""
import ctypes as C
import re

import pytest

import limits_utils as LU
from parity_utils import Both, reads_from_set

pytestmark = pytest.mark.gpu
FLAGS = pytest.mark.parametrize("flags", LU.FLAG_SETS, ids=LU.flag_id)


@pytest.fixture(scope="module")
def lib():
    from specimux_amd import _lib
    lib = _lib.load()
    n = C.c_int(0)
    _lib.check(lib.smx_device_init(0, C.byref(n)))
    assert n.value >= 1
    return lib


class OnceBoth(Both):
    """Both whose oracle records are computed once per (panel, flags, batch): the environment switches a case runs under
    change the kernel's plan, never the expected records."""
    _memo = {}

    def __init__(self, pf, sf, **flags):
        super().__init__(pf, sf, **flags)
        self._key = (pf, sf, tuple(sorted(flags.items())))

    def oracle_ops(self, reads):
        key = self._key + (id(reads), len(reads))
        if key not in self._memo:
            self._memo[key] = (reads, super().oracle_ops(reads))   # (the batch is kept alive: its id stays its own)
        return self._memo[key][1]


def check(pf, sf, flags, reads, label, want, sample=60):
    """Plan first (host), then both hit dumps of a sample and the records of every read."""
    from specimux_amd.demultiplex import compiled_panel
    both = OnceBoth(pf, sf, **flags)
    cp = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
    plan = cp.plan()
    LU.assert_fits(plan, label)
    want(plan, cp)
    if sample:
        step = max(1, len(reads) // sample)
        both.assert_hits_equal(list(dict.fromkeys(reads[::step] + reads[-3:])), label)   # (the last reads too: f puts flagged ones there)
    both.assert_ops_equal(reads, label)
    return plan


def overflow_tiles(capfd):
    """(tiles left to the redo launch, tiles) summed over the compact launches since the last call (SMX_DEBUG_OVERFLOW)."""
    got = re.findall(r"compact launch: (\d+) of (\d+) tiles left to the redo launch", capfd.readouterr().err)
    return sum(int(a) for a, _b in got), sum(int(b) for _a, b in got)


# ------------------------------------------------------------------ e. odd windows
@pytest.mark.parametrize("S", (1, 2) + LU.E_WINDOWS)
def test_odd_windows(lib, tmp_path_factory, S):
    sheet = LU.memo(LU.odd_window_sheet)
    pf, sf = LU.written(sheet, tmp_path_factory)
    reads = LU.memo(LU.odd_window_reads, sheet)
    for fl in LU.FLAG_SETS:
        check(pf, sf, dict(LU.E_BASE, search_len=S, **fl), reads, f"S {S} {fl}", lambda plan, cp: LU.e_want(plan, S))


@pytest.mark.parametrize("n", [1, 5, 65])
def test_odd_window_small_batches(lib, tmp_path_factory, n):
    sheet = LU.memo(LU.odd_window_sheet)
    pf, sf = LU.written(sheet, tmp_path_factory)
    reads = LU.memo(LU.odd_window_reads, sheet)[:n]
    for fl in LU.FLAG_SETS:
        check(pf, sf, dict(LU.E_BASE, search_len=17, **fl), reads, f"S 17, {n} reads {fl}", lambda plan, cp: LU.e_want(plan, 17), sample=n)


@pytest.fixture(scope="module")
def synth_panels(tmp_path_factory):
    from specimux_amd import synth
    out = {}
    for name in ("c2", "c3"):
        pan = getattr(synth, "panel_" + name)()
        out[name] = (pan, pan.write(str(tmp_path_factory.mktemp("lim_" + name))))
    return out


def test_odd_window_c2_at_255(lib, synth_panels):
    from specimux_amd import synth
    pan, (pf, sf) = synth_panels["c2"]
    rs = synth.make_reads(pan, 240, 255, search_len=255, windows_only=False)
    reads = reads_from_set(rs, range(240), 255)
    for fl in LU.FLAG_SETS:
        check(pf, sf, dict(search_len=255, **fl), reads, f"c2 S 255 {fl}", lambda plan, cp: LU.e_want(plan, 255))


# ------------------------------------------------------------------ f. tiles of 1, 2 and 4 reads on an ordinary panel
@pytest.mark.parametrize("name", ["c2", "c3"])
@pytest.mark.parametrize("r", LU.F_TILES)
def test_small_tiles(lib, synth_panels, monkeypatch, name, r):
    """Separates "small tile" from "large panel" when a case of a or b fails.  130 reads, a flagged read (short, N, lower
    case) first and last."""
    import random
    from specimux_amd import synth
    pan, (pf, sf) = synth_panels[name]
    rs = synth.make_reads(pan, 124, 600 + r, windows_only=False, **({} if name == "c2" else dict(insert_mean=900, insert_sd=250)))
    rng = random.Random(r)
    _pool, _fn, fs, _rn, rsq = pan.pools[0]
    flagged = LU.with_quals(LU.flagged_reads(pan.fwd[0], fs, pan.rev[0], rsq, rng, "first") +
                            LU.flagged_reads(pan.fwd[1], fs, pan.rev[1], rsq, rng, "last"), r)
    reads = flagged[:3] + reads_from_set(rs, range(124), 80) + flagged[3:]
    assert len(reads) == 130
    for env in LU.f_envs(r):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            for fl in LU.FLAG_SETS:
                check(pf, sf, fl, reads, f"{name} {env} {fl}", lambda plan, cp: LU.f_want(plan, r, env, len(cp.primers)), sample=30)


# ------------------------------------------------------------------ d. primer word edges
@pytest.mark.parametrize("S", LU.D_WINDOWS)
@pytest.mark.parametrize("m", LU.D_LENGTHS)
def test_primer_word_edges(lib, tmp_path_factory, m, S):
    rows = set()
    for variant, base in LU.D_PANELS:
        sheet = LU.memo(LU.primer_edge_sheet, m, variant)
        pf, sf = LU.written(sheet, tmp_path_factory)
        reads, _fam = LU.memo(LU.primer_edge_reads, sheet, m, S)
        for flags in LU.FLAG_SETS:
            fl = dict(base, **flags)
            plan = check(pf, sf, dict(fl, search_len=S), reads, f"{m} nt {variant} S {S} {fl}",
                         lambda plan, cp: LU.d_want(plan, m, variant, fl), sample=30)
            rows.add(plan.lean.variant)
    if m > 32:
        assert rows == {(64, b, 0, 0) for b in range(4)}, rows


# ------------------------------------------------------------------ a. many primers
@FLAGS
@pytest.mark.parametrize("env", LU.A_ENVS)
@pytest.mark.parametrize("n_pools", LU.A_POOLS)
def test_many_primers(lib, tmp_path_factory, monkeypatch, capfd, n_pools, env, flags):
    sheet = LU.memo(LU.many_primers_sheet, n_pools)
    pf, sf = LU.written(sheet, tmp_path_factory)
    reads, _fam = LU.memo(LU.many_primers_reads, sheet, n_pools)
    for k, v in LU.a_env(env, n_pools).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SMX_DEBUG_OVERFLOW", "1")
    capfd.readouterr()
    check(pf, sf, dict(LU.A_BASE, **flags), reads, f"{n_pools} pools {env} {flags}", lambda plan, cp: LU.a_want(plan, cp, n_pools, env, flags),
          sample=40)
    left, tiles = overflow_tiles(capfd)
    print(f"{n_pools} pools {env} {flags}: {left} of {tiles} compact tiles left to the redo launch")
    if env in ("dense", "no_prescan"):
        assert tiles == 0
    else:           # the redo launch did work: the batch's first tile cannot fit (many_primers_reads)
        assert tiles > 0 and left > 0, (left, tiles)
    if env == "overflow":
        # a compact tile holds 2 NP records: one read with an N (every alignment of it takes a record) and one matched
        # alignment of any other read are more; the batch has such a read in nearly every tile
        assert 2 * left > tiles, (left, tiles)


# ------------------------------------------------------------------ c. long barcodes, large k
@FLAGS
@pytest.mark.parametrize("L,k,caps", LU.C_CELLS)
def test_long_barcodes(lib, tmp_path_factory, monkeypatch, L, k, caps, flags):
    pf, sf = LU.written(LU.memo(LU.long_barcodes_sheet, L), tmp_path_factory)
    reads, _fam = LU.memo(LU.c_reads, L, k, pf, sf)
    if caps:
        monkeypatch.setenv("SMX_TEST_CAPS", caps)
    check(pf, sf, dict(LU.c_base(k), **flags), reads, f"{L} nt k {k} caps {caps} {flags}", lambda plan, cp: LU.c_want(plan, cp, L, k, caps))


# ------------------------------------------------------------------ b. many barcodes on one primer (1000 last)
@FLAGS
@pytest.mark.parametrize("k", LU.B_KS)
@pytest.mark.parametrize("maxB", sorted(LU.B_SIZES))
def test_many_barcodes(lib, tmp_path_factory, maxB, k, flags):
    pf, sf = LU.written(LU.memo(LU.many_barcodes_sheet, maxB)[0], tmp_path_factory)
    reads, _fam = LU.memo(LU.b_reads, maxB, k)
    check(pf, sf, dict(LU.b_base(k), **flags), reads, f"maxB {maxB} k {k} {flags}", lambda plan, cp: LU.b_want(plan, cp, maxB, k, flags),
          sample=40)
