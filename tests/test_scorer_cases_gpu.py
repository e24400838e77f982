"""The demux scorer (phase 4 of the demux kernel: score_fast, score_general, emit_op, specimen_exact, specimens_for) against
the oracle on the hand-written panels of tests/scorer_utils.py: sparse sheets, wildcards, two primers that match one
window, duplicate barcode pairs, one primer sequence under two names, 36 primer pairs.  tests/test_scorer_cases_cpu.py
checks, with the oracle alone, that the constructed reads hold at least 8 of every scorer situation on every panel and
flag set; here every record the kernel writes for them must equal the oracle's (run on the MI355X box: `pytest -m gpu`)."""
import ctypes as C
import os
from collections import Counter

import pytest

import scorer_utils as SU
from oracle import specimux_oracle as O
from parity_utils import RT, Both

pytestmark = pytest.mark.gpu

PANEL_NAMES = list(SU.PANELS)
FLAG_NAMES = list(SU.FLAG_SETS)


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
    return {name: pan.write(os.fspath(tmp_path_factory.mktemp(name))) for name, pan in SU.PANELS.items()}


_READS, _ORACLE = {}, {}


def reads_of(name):
    if name not in _READS:
        _READS[name] = SU.make_reads(SU.PANELS[name])
    return _READS[name]


def oracle_side(panel_files, name, flags, want_labels=False):
    """The oracle's records of a panel's constructed reads under one flag set, computed once per module and left unchanged."""
    key = (name, tuple(sorted(flags.items())))
    if key not in _ORACLE:
        pf, sf = panel_files[name]
        panel, par = SU.oracle_setup(pf, sf, **flags)
        ops, total, matched = O.process_sequences(reads_of(name), par, panel)
        keys = [(op.seq_id, op.sample_id, op.code, op.pool, op.p1, op.p2, RT[op.rtype], op.sequence, op.quality) for op in ops]
        _ORACLE[key] = dict(ops=ops, keys=keys, total=total, matched=matched, panel=panel, par=par)
    side = _ORACLE[key]
    if want_labels and "labels" not in side:
        side["counts"], side["labels"] = SU.census(side["par"], side["panel"], reads_of(name), ops=side["ops"])
    return side


def both_for(panel_files, name, flags):
    """parity_utils.Both whose oracle side is the cached one (assert_ops_equal then runs the product only)."""
    pf, sf = panel_files[name]
    both = Both(pf, sf, **flags)
    side = oracle_side(panel_files, name, flags)
    reads = reads_of(name)

    def cached(rs):
        assert rs is reads, "the cached oracle records belong to the panel's constructed reads"
        return side["keys"], side["total"], side["matched"]
    both.oracle_ops = cached
    return both, side


def by_read(keys):
    out = {}
    for k in keys:
        out.setdefault(k[0], []).append(k)
    return out


# ------------------------------------------------------------------ records and hit tables, every panel x flag set
@pytest.mark.parametrize("fname", FLAG_NAMES)
@pytest.mark.parametrize("name", PANEL_NAMES)
def test_records_equal_oracle(lib, panel_files, name, fname):
    flags = SU.FLAG_SETS[fname]
    both, side = both_for(panel_files, name, flags)
    reads = reads_of(name)
    got = both.assert_ops_equal(reads, f"{name} {fname}")
    assert len(got) == len(side["keys"]) >= len(reads)
    if flags.get("dereplicate") == "none" and name == "multi":
        assert max(Counter(k[0] for k in got).values()) >= 8      # one read, eight records (both variants x both orientations)
    step = len(reads) // 60
    both.assert_hits_equal(reads[::step][:60], f"{name} {fname}")


# ------------------------------------------------------------------ counters, locations, batch order
def _run_counts(both, reads):
    from specimux_amd.demultiplex import compiled_panel, concat_records
    from specimux_amd.io_utils import SeqRecord
    cp = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
    bases, offsets, _ = concat_records([SeqRecord(s, rid, rid, q) for rid, s, q in reads])
    windows, lens = cp.pack_windows(bases, offsets)
    _ops, _extra, counts = cp.run(windows, lens)
    return cp, counts


@pytest.mark.parametrize("fname", ["default", "derep_none"])
@pytest.mark.parametrize("name", PANEL_NAMES)
def test_counters_equal_a_tally_of_the_oracles_records(lib, panel_files, name, fname):
    """smx_batch_run's counters against a tally of the oracle's records: per specimen (records of class full -- FULL,
    MULTIPLE, DEREP -- that name it; a trim-to-empty fallback record names none), and the totals."""
    from specimux_amd import _lib
    both, side = both_for(panel_files, name, SU.FLAG_SETS[fname])
    reads = reads_of(name)
    cp, counts = _run_counts(both, reads)
    ops = side["ops"]
    full = [op for op in ops if op.rtype in (O.R_FULL, O.R_MULTI, O.R_DEREP)]
    per = Counter(op.sample_id for op in full)
    assert sum(per.values()) > 100 and len(per) >= 5
    for i, sid in enumerate(cp.specimen_ids):
        assert int(counts[_lib.CNT_SPECIMEN0 + i]) == per.get(sid, 0), (name, fname, sid)
    assert int(counts[_lib.CNT_TOTAL]) == len(reads) and int(counts[_lib.CNT_FILTERED]) == 0
    assert int(counts[_lib.CNT_MATCHED]) == side["matched"]
    assert int(counts[_lib.CNT_OPS_FULL]) == len(full)
    assert int(counts[_lib.CNT_OPS_PARTIAL]) == sum(1 for op in ops if op.rtype in (O.R_PFWD, O.R_PREV))
    assert int(counts[_lib.CNT_OPS_UNKNOWN]) == sum(1 for op in ops if op.rtype == O.R_UNKNOWN)
    assert int(counts[_lib.CNT_MULTI_OP_READS]) == sum(1 for n in Counter(op.seq_id for op in ops).values() if n > 1)
    assert int(counts[_lib.CNT_OVERFLOW]) == 0


@pytest.mark.parametrize("flags", [dict(), dict(trim="primers")], ids=["default", "trim_primers"])
def test_locations_multi(lib, panel_files, flags):
    pf, sf = panel_files["multi"]
    both = Both(pf, sf, **flags)
    assert both.assert_locations_equal(reads_of("multi"), f"multi {flags}") > 1000


@pytest.mark.parametrize("fname", ["default", "derep_none"])
@pytest.mark.parametrize("name", PANEL_NAMES)
def test_batch_order_does_not_change_a_reads_records(lib, panel_files, name, fname):
    """The same reads as built, reversed and sorted by situation: a read's records may not depend on its tile neighbours
    or on what the previous tile left in the LDS regions the scorer reuses (the running trim shifts, the match masks)."""
    flags = SU.FLAG_SETS[fname]
    pf, sf = panel_files[name]
    side = oracle_side(panel_files, name, flags, want_labels=True)
    reads = reads_of(name)
    exp = by_read(side["keys"])
    labels = side["labels"]
    orders = {"as built": reads, "reversed": reads[::-1], "by situation": sorted(reads, key=lambda r: (labels[r[0]], r[0]))}
    both = Both(pf, sf, **flags)
    for label, rs in orders.items():
        keys, total, matched = both.product_ops(rs)
        assert (total, matched) == (side["total"], side["matched"]), label
        got = by_read(keys)
        bad = [rid for rid in exp if got.get(rid) != exp[rid]]
        assert not bad and len(got) == len(exp), f"{name} {fname} {label}: {len(bad)} read(s) differ, first {bad[:1]}: " \
            f"gpu {[k[1:7] for k in got.get(bad[0], [])] if bad else ''} oracle {[k[1:7] for k in exp[bad[0]]] if bad else ''}"
        assert [k[0] for k in keys] == [r[0] for r in rs for _ in exp[r[0]]], label      # records in read order


# ------------------------------------------------------------------ every scorer variant
VARIANTS = {
    "default": {},                                          # the library's own choice
    "generic": {"SMX_NO_SPECIALISE": "1"},                  # the generic instantiation
    "dense": {"SMX_COMPACT": "0"},                          # dense tiles
    "overflow": {"SMX_COMPACT_ITEMS": "16"},                # compact tiles with an overflow list and the redo launch
    "two_lanes": {"SMX_COMPACT": "0", "SMX_TILE_R": "32"},  # two lanes per read in score_fast
    "four_lanes": {"SMX_COMPACT": "0", "SMX_TILE_R": "16"}, # four lanes per read in score_fast
}


@pytest.mark.parametrize("fname", ["default", "derep_none"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["multi", "two_pairs"])
def test_scorer_variants(lib, panel_files, monkeypatch, name, variant, fname):
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)      # read when the panel is compiled: both_for builds a fresh one
    both, _side = both_for(panel_files, name, SU.FLAG_SETS[fname])
    both.assert_ops_equal(reads_of(name), f"{name} {variant} {fname}")
