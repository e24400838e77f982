"""The demux kernel's per-read primer search (primer_item in smx_demux_tile.h, fed by prescan_decode) against the oracle on the
panels and constructed reads of tests/primer_utils.py: primer lengths at the word-size edges (31, 32, 33, 63, 64 nt), the
panels whose whole search falls back (five degenerate letters, SMX_NO_PRESCAN, one long primer among eight), the primer in
every window column, cut at the window's inner edge, twice in a row, at exactly k and k + 1 edits, reads of every
end_geom length and reads with bytes that are not upper-case ACGT.  tests/test_primer_cases_cpu.py checks, with the oracle
alone, that every cell holds enough of each case; here the hit table of EVERY constructed read (both dumps: pdist, nloc,
first_end, with trimming first_start) and every record must equal the oracle's (run on the MI355X box: `pytest -m gpu`).

The oracle's aligner (oracle/align_oracle.c) is a plain int DP: it has no word size and no window chunks."""
import ctypes as C
import os

import pytest

import primer_utils as PU
from oracle import specimux_oracle as O
from parity_utils import RT, Both, reads_from_set

pytestmark = pytest.mark.gpu

FLAG_SETS = {"default": dict(), "trim_primers": dict(trim="primers"), "trim_tails": dict(trim="tails"),
             "no_preorient": dict(disable_preorient=True)}


@pytest.fixture(scope="module")
def lib():
    from specimux_amd import _lib
    lib = _lib.load()
    n = C.c_int(0)
    _lib.check(lib.smx_device_init(0, C.byref(n)))
    assert n.value >= 1
    return lib


@pytest.fixture(scope="module")
def panel_files(tmp_path_factory):
    files = {}

    def get(name):
        if name not in files:
            files[name] = PU.PANELS[name]().write(os.fspath(tmp_path_factory.mktemp(name)))
        return files[name]
    return get


_ORACLE, _TABLES = {}, {}
_hit_table = O.hit_table


def _memo_hit_table(scope):
    """O.hit_table, computed once per read of a cell (it depends on the thresholds and the window, which the four flag
    sets and the environment variants of a cell share) and left unchanged."""
    def hit_table(par, panel, rec, prefilter="auto"):
        key = (scope, par.search_len, rec[0])
        if key not in _TABLES:
            _TABLES[key] = _hit_table(par, panel, rec, prefilter)
        return _TABLES[key]
    return hit_table


def both_for(panel_files, monkeypatch, name, S, flags, reads, scope, tscope=None):
    """parity_utils.Both with the oracle's records of `reads` computed once per (scope, flag set)."""
    pf, sf = panel_files(name)
    both = Both(pf, sf, search_len=S, **flags)
    key = (scope, S, tuple(sorted(flags.items())))
    if key not in _ORACLE:
        ops, total, matched = O.process_sequences(reads, both.opar, both.opanel)
        keys = [(op.seq_id, op.sample_id, op.code, op.pool, op.p1, op.p2, RT[op.rtype], op.sequence, op.quality) for op in ops]
        _ORACLE[key] = (reads, keys, total, matched)
    side = _ORACLE[key]

    def cached(rs):
        assert rs is side[0], "the cached oracle records belong to these reads"
        return side[1:]
    both.oracle_ops = cached
    monkeypatch.setattr(O, "hit_table", _memo_hit_table(tscope or scope))
    return both


def compile_or_unsupported(both):
    """The compiled panel, or None after a loud SMX_ERR_UNSUPPORTED from panel creation (the one acceptable way for the
    library to decline a shape its tile plan cannot hold)."""
    from specimux_amd import _lib
    from specimux_amd.demultiplex import compiled_panel
    try:
        return compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
    except _lib.SmxError as e:
        assert e.code == _lib.ERR_UNSUPPORTED, e
        assert "bytes of LDS per read tile" in str(e), e
        return None


# ------------------------------------------------------------------ every cell x flag set, all constructed reads
@pytest.mark.parametrize("fname", list(FLAG_SETS))
@pytest.mark.parametrize("cell", PU.CELLS, ids=PU.cell_id)
def test_primer_search_equals_oracle(lib, panel_files, monkeypatch, cell, fname):
    name, S, env, _path = cell
    for k, v in env.items():
        monkeypatch.setenv(k, v)      # read when the panel is compiled: Both builds a fresh one
    reads = PU.cell(name, S).reads
    both = both_for(panel_files, monkeypatch, name, S, FLAG_SETS[fname], reads, name)
    label = f"{PU.cell_id(cell)} {fname}"
    if name == "c3_m33" and compile_or_unsupported(both) is None:
        return
    checked = both.assert_hits_equal(reads, label)
    assert checked >= 20, (label, checked)
    assert both.assert_ops_equal(reads, label)


# ------------------------------------------------------------------ read kind against batch position
def _batch(name, S=80):
    """1 317 reads = one full 1024-read tile + one full 256-read sub-tile + a 37-read partial sub-tile: clean synthetic
    filler, with the cell's dirty reads and its reads shorter than the window on the sub-tile edge (254-257), on the tile
    edge (1022-1025) and in all of the last 37 slots."""
    from specimux_amd import synth
    cell = PU.cell(name, S)
    n = 1317
    rs = synth.make_reads(cell.panel, n, 4711, search_len=S, windows_only=False)
    batch = reads_from_set(rs, range(n), S, prefix="fill")
    dirty = [r for r in cell.reads if cell.meta[r[0]]["dirty"]]
    short = [r for r in cell.reads if 0 < len(r[1]) < S]
    special = [r for pair in zip(dirty[::max(1, len(dirty) // 23)], short[::max(1, len(short) // 23)]) for r in pair][:45]
    assert len(special) == 45 and len({r[0] for r in special}) == 45
    slots = list(range(254, 258)) + list(range(1022, 1026)) + list(range(n - 37, n))
    for i, r in zip(slots, special):
        batch[i] = r
    assert all(not set(r[1]) <= set("ACGT") or len(r[1]) < S for r in (batch[i] for i in slots))
    return batch


@pytest.mark.parametrize("order", ["as_built", "reversed"])
@pytest.mark.parametrize("name", ["m22", "m32"])
def test_read_kind_against_batch_position(lib, panel_files, monkeypatch, name, order):
    """The prescan's transpose takes 256 reads per sub-tile and 1024 per tile and routes reads that are short or hold
    anything but upper-case ACGT to the demux kernel's ASCII path by their naflag byte: such reads on a sub-tile edge, on
    a tile edge and filling the partial last sub-tile (the transpose's bounds branch), then the same batch reversed, so
    that the partial sub-tile holds other reads.  Records and hit tables of every read of the batch."""
    batch = _batch(name)
    if order == "reversed":
        batch = batch[::-1]
    _BATCHES.setdefault((name, order), batch)
    batch = _BATCHES[(name, order)]
    both = both_for(panel_files, monkeypatch, name, 80, {}, batch, f"batch/{name}/{order}", tscope=f"batch/{name}")
    both.assert_ops_equal(batch, f"batch {name} {order}")
    both.assert_hits_equal(batch, f"batch {name} {order}")


_BATCHES = {}
