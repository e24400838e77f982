"""The demux kernel's tile loop (smx_demux_tile.h: pop_tile, phase1_encode; smx_scorer.h: emit_op, specimen records) on the GPU, at the batch
sizes and read mixes where the loop takes another path: one, two and three 64-read tiles, a last tile whose size is not a
multiple of four (the dword-per-lane encode instead of the 16-byte one), an empty next tile, reads the prescan flags (shorter
than the window, an N, a lower-case base) at every position of a group of four in the first and in the last tile, batches of
nothing but flagged reads, and a launch in which every workgroup walks many tiles.  Records against the CPU oracle through
parity_utils; the 100 000-read launch also against the generic instantiation, byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import scorer_utils as SU
from parity_utils import Both, reads_from_set

pytestmark = pytest.mark.gpu

BATCH_SIZES = [1, 3, 4, 5, 63, 64, 65, 66, 129]
KINDS = ("short", "n", "lower")
N_BASE = 144          # two full tiles and a last tile of up to 16 reads
EXTRA_ORDER = ["read", "sample", "trim_start", "p1", "p2", "barcode", "rtype"]


@pytest.fixture(scope="module")
def lib():
    from specimux_amd import _lib
    lib = _lib.load()
    n = C.c_int(0)
    _lib.check(lib.smx_device_init(0, C.byref(n)))
    assert n.value >= 1
    return lib


def _flag(read, kind, i):
    """`read` as the prescan flags it: cut below the window length, an N in the head window, a lower-case base in the tail
    window"""
    rid, s, q = read
    if kind == "short":
        L = 24 + (i * 13) % 56
        return f"{rid}_short", s[:L], q[:L]
    if kind == "n":
        pos = (i * 11) % 80
        return f"{rid}_n", s[:pos] + "N" + s[pos + 1:], q
    pos = len(s) - 80 + (i * 7) % 80
    return f"{rid}_lower", s[:pos] + s[pos].lower() + s[pos + 1:], q


class Panel:
    """One panel's files, N_BASE clean reads (at least 160 nt, upper-case ACGT), every flagged form of each, a few reads
    without any primer, and the oracle's records of all of them per read id (a read's records do not depend on its batch),
    computed once."""

    def __init__(self, files, base, flags=None):
        self.files, self.base = files, base
        assert len(base) == N_BASE and all(len(s) >= 160 and set(s) <= set("ACGT") for _r, s, _q in base)
        self.flagged = {k: [_flag(r, k, i) for i, r in enumerate(base)] for k in KINDS}
        rng = np.random.default_rng(77)
        self.junk = [(f"junk{i}", "".join("ACGT"[b] for b in rng.integers(0, 4, 300)), "I" * 300) for i in range(8)]
        self._oracle = {}

    def oracle(self, **flags):
        key = tuple(sorted(flags.items()))
        if key not in self._oracle:
            everything = self.base + [r for k in KINDS for r in self.flagged[k]] + self.junk
            keys, _t, _m = Both(*self.files, **flags).oracle_ops(everything)
            by = {}
            for k in keys:
                by.setdefault(k[0], []).append(k)
            self._oracle[key] = by
        return self._oracle[key]

    def batch(self, n, flagged=()):
        """the first n base reads, read i replaced by its flagged form `kind` for every (i, kind) in `flagged`"""
        out = list(self.base[:n])
        for i, kind in flagged:
            out[i] = self.flagged[kind][i]
        return out


@pytest.fixture(scope="module")
def panels(tmp_path_factory):
    from specimux_amd import synth
    out = {}
    for name, pan in (("c2", synth.panel_c2()), ("c3", synth.panel_c3())):
        files = pan.write(os.fspath(tmp_path_factory.mktemp(name + "loop")))
        rs = synth.make_reads(pan, 400, 6161, windows_only=False)
        reads = [r for r in reads_from_set(rs, range(400), 80) if len(r[1]) >= 160 and set(r[1]) <= set("ACGT")]
        out[name] = Panel(files, reads[:N_BASE])
    pan = SU.PANELS["one_pair_sparse"]
    files = pan.write(os.fspath(tmp_path_factory.mktemp("sparseloop")))
    reads = [r for r in SU.make_reads(pan) if len(r[1]) >= 160 and set(r[1]) <= set("ACGT")]
    out["one_pair_sparse"] = Panel(files, reads[::len(reads) // N_BASE][:N_BASE])   # a spread over the constructed families
    return out


def _both(panel, env=None, **flags):
    """parity_utils.Both created under the given switches (a panel reads them once, when it is compiled: on its first batch)"""
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        both = Both(*panel.files, **flags)
        both.product_ops(panel.base[:1])
        return both
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _check(both, panel, reads, label, **flags):
    got, total, _matched = both.product_ops(reads)
    assert total == len(reads), label
    exp = panel.oracle(**flags)
    by = {}
    for k in got:
        by.setdefault(k[0], []).append(k)
    assert len(by) == len(reads), label
    for rid, _s, _q in reads:
        assert by.get(rid) == exp[rid], f"{label}: read {rid}:\n  gpu    {[k[1:7] for k in by.get(rid, [])]}\n  oracle {[k[1:7] for k in exp[rid]]}"
    assert [k[0] for k in got] == [r[0] for r in reads for _ in exp[r[0]]], f"{label}: records out of read order"


_BOTH = {}


def _default(lib, panels, name):
    if name not in _BOTH:
        _BOTH[name] = _both(panels[name])
    return _BOTH[name]


# ------------------------------------------------------------------ batch sizes
@pytest.mark.parametrize("n", BATCH_SIZES)
@pytest.mark.parametrize("name", ["one_pair_sparse", "c2"])
def test_batch_sizes(lib, panels, name, n):
    """clean reads, and the same batch with one read of every flagged kind in it (where it holds three reads)"""
    both, p = _default(lib, panels, name), panels[name]
    _check(both, p, p.batch(n), f"{name} n={n}")
    if n >= 3:
        mixed = [(n - 1, "short"), (n // 2, "n"), (0, "lower")]
        _check(both, p, p.batch(n, mixed), f"{name} n={n} mixed")


# ------------------------------------------------------------------ flagged reads
@pytest.mark.parametrize("n", [143, 144], ids=["last_tile_15", "last_tile_16"])
@pytest.mark.parametrize("pos", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["one_pair_sparse", "c2"])
def test_flagged_read_at_every_position_of_a_group_of_four(lib, panels, name, pos, n):
    """One flagged read of each kind at position `pos` mod 4, in the first tile and in the last one.  143 reads: the last tile
    holds 15 and takes the dword-per-lane encode; 144: it holds 16 and takes the 16-byte encode like the full tiles."""
    both, p = _default(lib, panels, name), panels[name]
    flagged = [(base + 4 * k + pos, kind) for base in (8, 128) for k, kind in enumerate(KINDS)]
    assert max(i for i, _k in flagged) < n
    _check(both, p, p.batch(n, flagged), f"{name} pos={pos} n={n}")


@pytest.mark.parametrize("n", [5, 64, 129])
@pytest.mark.parametrize("name", ["one_pair_sparse", "c2"])
def test_every_read_flagged(lib, panels, name, n):
    both, p = _default(lib, panels, name), panels[name]
    _check(both, p, p.batch(n, [(i, KINDS[i % 3]) for i in range(n)]), f"{name} all flagged n={n}")


# ------------------------------------------------------------------ variants
VARIANTS = {
    "generic": dict(env={"SMX_NO_SPECIALISE": "1"}),
    "planes": dict(env={"SMX_PRESCAN_PLANES": "1"}),            # row-major codes: the dword-per-lane encode on every tile
    "generic_planes": dict(env={"SMX_NO_SPECIALISE": "1", "SMX_PRESCAN_PLANES": "1"}),
    "derep_none": dict(env={}, flags=dict(dereplicate="none")),   # with reads that have no candidate at all (best == 0)
}


@pytest.mark.parametrize("n", [5, 66, 129])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["one_pair_sparse", "c2"])
def test_variants(lib, panels, name, variant, n):
    v = VARIANTS[variant]
    flags = v.get("flags", {})
    p = panels[name]
    both = _both(p, v["env"], **flags)
    reads = p.batch(n, [(n - 1, "short"), (n // 2, "n"), (1, "lower")])
    if variant == "derep_none":
        for k, i in enumerate([0, n - 2] + ([n // 2 + 1] if n > 8 else [])):   # (not the flagged positions)
            reads[i] = p.junk[k]
    _check(both, p, reads, f"{name} {variant} n={n}", **flags)


@pytest.mark.parametrize("items", [None, "40"], ids=["compact", "compact_40_items"])
def test_compact_and_redo_launch(lib, panels, items):
    """c3 (eight primers) runs a compact launch and a redo launch.  By default the tiles of this batch fit their records and
    the redo launch finds an empty list: every workgroup of it leaves before it stages the panel.  With 40 records per tile
    the tiles overflow and the redo launch does the work."""
    p = panels["c3"]
    both = _both(p, {"SMX_COMPACT_ITEMS": items} if items else {})
    for n in (66, 129):
        _check(both, p, p.batch(n, [(n - 1, "short"), (n // 2, "n"), (1, "lower")]), f"c3 items={items} n={n}")


# ------------------------------------------------------------------ many tiles per workgroup
def test_many_tiles_per_workgroup(lib, panels, tmp_path_factory):
    """100 000 c2 reads with one workgroup per CU: 1563 tiles for 256 workgroups, about six each, so every workgroup pops,
    encodes and scores several tiles in a row and ends on an empty pop.  The default and the generic instantiation must
    write the same bytes; the counters must add up to the records; and a fixed sample of 4 000 reads must equal the oracle:
    the sample's records in the large launch equal its records as a batch of its own (all fields but the read index), and
    that batch is compared with the oracle read by read."""
    from specimux_amd import _lib, synth
    from specimux_amd.demultiplex import compiled_panel
    p = panels["c2"]
    n = 100_000
    rs = synth.make_reads(synth.panel_c2(), n, 4242)
    runs = {}
    for label, env in (("default", {"SMX_BLOCKS_PER_CU": "1"}), ("generic", {"SMX_BLOCKS_PER_CU": "1", "SMX_NO_SPECIALISE": "1"})):
        both = _both(p, env)
        cp = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
        windows, lens = rs.windows(cp.window_stride), rs.lens
        ops, extra, counts = cp.run(windows, lens)
        runs[label] = (both, cp, ops, np.sort(extra, order=EXTRA_ORDER), counts)
    (both, cp, ops, extra, counts), (_b, _c, gops, gextra, gcounts) = runs["default"], runs["generic"]
    assert ops.tobytes() == gops.tobytes(), "records differ between the default and the generic instantiation"
    assert extra.tobytes() == gextra.tobytes() and np.array_equal(counts, gcounts)
    # counter identities
    everything = np.concatenate([ops, extra])
    rt = everything["rtype"]
    full = np.isin(rt, (_lib.R_FULL, _lib.R_MULTIPLE, _lib.R_DEREP_FULL))
    assert np.array_equal(ops["read"], np.arange(n, dtype=np.uint32))
    assert int(counts[_lib.CNT_TOTAL]) == n and int(counts[_lib.CNT_FILTERED]) == 0 and int(counts[_lib.CNT_OVERFLOW]) == 0
    assert int(ops["n_ops"].astype(np.int64).sum()) == len(everything)
    assert int(counts[_lib.CNT_OPS_FULL]) == int(full.sum()) > n // 2
    assert int(counts[_lib.CNT_OPS_PARTIAL]) == int(np.isin(rt, (_lib.R_PARTIAL_FWD, _lib.R_PARTIAL_REV)).sum())
    assert int(counts[_lib.CNT_OPS_UNKNOWN]) == int((rt == _lib.R_UNKNOWN).sum())
    assert int(counts[_lib.CNT_OPS_FULL] + counts[_lib.CNT_OPS_PARTIAL] + counts[_lib.CNT_OPS_UNKNOWN]) == len(everything)
    assert int(counts[_lib.CNT_MULTI_OP_READS]) == int((ops["n_ops"] > 1).sum())
    assert int(counts[_lib.CNT_MATCHED]) == len(np.unique(everything["read"][np.isin(rt, (_lib.R_FULL, _lib.R_DEREP_FULL))]))
    per = np.bincount(everything["sample"][full & (everything["sample"] >= 0)], minlength=cp.counts_len - _lib.CNT_SPECIMEN0)
    assert np.array_equal(counts[_lib.CNT_SPECIMEN0:].astype(np.int64), per) and int(per.sum()) == int(full.sum())
    # the sample
    idx = np.sort(np.random.default_rng(4243).choice(n, 4000, replace=False))
    sops, sextra, _sc = cp.run(np.ascontiguousarray(windows[idx]), np.ascontiguousarray(lens[idx]))
    for f in ops.dtype.names:
        if f != "read":
            assert np.array_equal(sops[f], ops[f][idx]), f"sample: field {f} of the primary records differs from the large launch"
    assert len(sextra) == int(np.isin(extra["read"], idx).sum())
    both.assert_ops_equal(reads_from_set(rs, idx, 80), "sample of the 100 000")
