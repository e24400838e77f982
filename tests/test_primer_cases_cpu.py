"""CPU side of the primer-search tests (no GPU needed): the census that keeps tests/test_primer_cases_gpu.py honest, and the
rules by which a panel selects the path of primer_item (smx_demux_tile.h) that a cell is meant to reach.

The census is computed with the oracle alone (tests/primer_utils.py): for every (panel, search_len) cell the constructed
reads must hold at least 4 matches that end in each 16-column chunk of the target, in its last column, that start in its
first column, that have adjacent optimal ends, optimal ends in two 32-column words, and that fall in each end_geom class;
and at least 8 each at distance 0, at the threshold k, one above it (rejected), and matched / unmatched among the reads
with a byte that is not upper-case ACGT.  What cannot occur in a cell is excluded by name, with the reason
(primer_utils.cannot):
  end_chunk[c], 16 c + 15 < need - 1   an alignment within k edits spends at least need = min over primers (m - k) target
                                       columns, so no match ends before column need - 1 (chunk 0 on the panels whose
                                       shortest primer is the 20-nt reverse primer is reachable: need = 14)
  S/2 < L <= S-2 and L <= S/2, S = 16  the target of such a read has at most 7 (8) columns, a match needs 14
  multi_two_words, S = 16              one 32-column word
  d0, S = 16                           both primers are longer than the window: at least m - 16 edits

The path rule is not visible from Python without a device (the panel is compiled by smx_panel_create); expected_path
restates it from smx_panel.cpp / smx_prescan_core.h and is checked here against the table of cells, the header's two
constants are read from the source."""
import pytest

import primer_utils as PU
from oracle import specimux_oracle as O


@pytest.mark.parametrize("name,S", PU.CENSUS_CELLS, ids=[f"{n}-S{S}" for n, S in PU.CENSUS_CELLS])
def test_census(name, S):
    cell = PU.cell(name, S)
    assert 500 <= len(cell.reads) <= 1520
    counts = PU.census(cell)
    cannot = PU.cannot(cell)
    chunks = [("end_chunk", c) for c in range((S + 15) // 16)]
    print(f"{name} S={S}: {len(cell.reads)} reads; end_chunk " + " ".join(str(counts[c]) for c in chunks) + "; " +
          ", ".join(f"{k} {counts[k]}" for k in PU.LABELS) + f"; cannot: {sorted(map(str, cannot))}")
    assert set(counts) <= set(chunks + PU.LABELS), set(counts) - set(chunks + PU.LABELS)
    for k in chunks + PU.LABELS:
        if k in cannot:
            assert counts[k] == 0, (name, S, k, counts[k], cannot[k])
        else:
            assert counts[k] >= (PU.MIN_READS if k in PU.AT_LEAST_8 else PU.MIN_HITS), (name, S, k, counts[k])
    # the exclusions are the ones the module docstring lists, nothing else
    if S >= 64:
        assert set(cannot) <= {("end_chunk", 0), ("end_chunk", 1)}, cannot
    if (name, S) == ("m22", 16):
        assert set(cannot) == {"S/2<L<=S-2", "L<=S/2", "multi_two_words", "d0"}


@pytest.mark.parametrize("name,S", [c for c in PU.CENSUS_CELLS if c[0] not in ("c3", "c3_m33")],
                         ids=[f"{n}-S{S}" for n, S in PU.CENSUS_CELLS if n not in ("c3", "c3_m33")])
def test_census_of_the_primer_the_cell_is_about(name, S):
    """The panel's longest primer -- the one whose length sits at the word-size edge -- itself has matches at distance 0
    and k, in the target's last column, starting in its first column and with adjacent optimal ends (the cell-wide census
    counts both primers)."""
    cell = PU.cell(name, S)
    panel = O.load_panel(*PU._written(cell))
    long_name = max(panel.primers.values(), key=lambda p: len(p.primer)).name
    counts = PU.census(cell, only=long_name)
    m = max(len(p.primer) for p in panel.primers.values())
    # (a window shorter than the primer leaves one spare edit: two reads tie there, and none is at distance 0)
    for k in ("end_last_col", "start_first_col", "d_eq_k") + (("d0", "multi_adjacent") if S >= m else ()):
        assert counts[k] >= PU.MIN_HITS, (name, S, long_name, k, counts[k])


def test_header_constants_of_the_restated_rule():
    assert PU._header_constant("PRE_MAXROWS") == 31 and PU._header_constant("PRE_MAXSYM") == 8


@pytest.mark.parametrize("cell", PU.CELLS, ids=PU.cell_id)
def test_cell_selects_the_path_it_means_to_test(cell):
    name, S, env, want = cell
    primers = PU.cell(name, S).primer_seqs()
    assert PU.expected_path(primers, S, env) == want
    lens = sorted({len(p) for p in primers})
    if name.startswith("m") and not env:
        assert max(lens) == int(name[1:3])
    if name == "deg5":      # refused for its letters alone: S = 80 is a multiple of 16, 23 nt fit the 31 rows
        assert max(lens) == 23 and PU.expected_path([p for p in primers if p != PU.DEG5], S, env) == "prescan<5>"
        assert PU.expected_path(["GAYGAYMGWGATCAYTTYGG"], S, env) == "prescan<5>"      # four letters are served
    if name == "c3_m33":    # one primer of eight forces the 64-bit words; without it the panel is the prescan's
        assert len(primers) == 8 and sorted(len(p) for p in primers)[-2:] == [23, 33]
        assert PU.expected_path(PU.cell("c3", 80).primer_seqs(), S, {}).startswith("prescan")


def test_rule_edges():
    its = "CTTGGTCATTTAGAGGAAGTAA"
    assert PU.expected_path([PU.LONG64[:31], its], 80, {}) == "prescan<5>"
    assert PU.expected_path([PU.LONG64[:32], its], 80, {}) == "unrolled u32"
    assert PU.expected_path([PU.LONG64[:32], its], 83, {}) == "generic u32"
    assert PU.expected_path([PU.LONG64[:33], its], 80, {}) == "generic u64"
    assert PU.expected_path([its], 84, {}) == "unrolled u32"
    assert PU.expected_path([its], 160, {}) == "prescan<10>" and PU.expected_path([its], 256, {}) == "prescan<0>"


def test_constructs_lie_where_the_docstring_says():
    """The sweep's exact primer ends in window column S - 1 - x - 13 (behind a barcode) or S - 1 - x (flush): checked on
    the oracle's hit table for both orientations of the m32 cell, whose 32-nt primer matches nowhere else."""
    cell = PU.cell("m32", 80)
    panel = O.load_panel(*PU._written(cell))
    par = O.setup_params(panel, search_len=80)
    seen = 0
    for rec in cell.reads:
        rid, s, _q = rec
        if not rid.startswith("sweep_"):
            continue
        x, bc = int(rid.split("_")[1][1:]), rid.split("_")[2] == "b"
        e = 79 - x - (13 if bc else 0)
        if e < 31:
            continue
        end = "A" if rid.endswith("f") else "B"
        h = PU.hit_table(cell, par, panel, rec)[("FWD", end)]
        assert h["pdist"] == 0 and h["locs"] == [(len(s) - 80 + e - 31, len(s) - 80 + e)], (rid, h)
        seen += 1
    assert seen >= 100
