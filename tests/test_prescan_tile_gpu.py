"""The primer prescan on tile codes (prescan_tilecodes_kernel, prescan_dp_kernel with TS = 1 and the demux kernel's tile-major
encode, smx_prescan.hip / smx_demux_tile.h) on the GPU: the two-primer panel at search_len 80, batches that mix full-length,
short and non-ACGT reads, at the read counts where a 32-read group, a 256-read sub-tile or a 1024-read DP tile is partial.
Records, totals and hit tables against the CPU oracle; records, extra records, counts and hit tables against the same batch
run with SMX_PRESCAN_PLANES=1 (the plane buffer and the row-major codes)."""
import ctypes as C
import os

import numpy as np
import pytest

from parity_utils import Both, reads_from_set, tmp_panel

pytestmark = pytest.mark.gpu

READ_COUNTS = [1, 31, 32, 33, 255, 257, 1023, 1025, 2049]
EXTRA_ORDER = ["read", "sample", "trim_start", "p1", "p2", "barcode", "rtype"]
HIT_FIELDS = ["pdist", "nloc", "first_end", "bbest", "ntied", "first_tied"]


@pytest.fixture(scope="module")
def lib():
    from specimux_amd import _lib
    lib = _lib.load()
    n = C.c_int(0)
    _lib.check(lib.smx_device_init(0, C.byref(n)))
    assert n.value >= 1
    return lib


@pytest.fixture(scope="module")
def c2(tmp_path_factory):
    from specimux_amd import synth
    pan = synth.panel_c2()
    return pan, tmp_panel(tmp_path_factory, pan, "c2tile")


@pytest.fixture(scope="module")
def reads(c2):
    """2049 reads, generated once and sliced by the tests.  Read 0 is short, read 1 carries an N in its head window, read 2
    an R in its tail window; after that every 7th read is one of the three in turn, so that every batch mixes them."""
    from specimux_amd import synth
    rs = synth.make_reads(c2[0], 2049, 5151, windows_only=False)
    out = reads_from_set(rs, range(2049), 80)
    for i in list(range(3)) + list(range(7, 2049, 7)):
        rid, s, q = out[i]
        kind = i % 3 if i < 3 else (i // 7) % 3
        if kind == 0:
            L = 20 + (i * 13) % 60
            s, q = s[:L], q[:L]
        elif len(s) >= 80:
            pos = (i * 11) % 80
            if kind == 1:
                s = s[:pos] + "N" + s[pos + 1:]
            else:
                s = s[:len(s) - 80 + pos] + "R" + s[len(s) - 80 + pos + 1:]
        out[i] = (rid, s, q)
    return out


@pytest.fixture(scope="module")
def oracle(c2, reads):
    """The oracle's records of all 2049 reads, per read (a read's records do not depend on the rest of its batch)."""
    _pan, (pf, sf) = c2
    keys, _total, _matched = Both(pf, sf).oracle_ops(reads)
    by = {}
    for k in keys:
        by.setdefault(k[0], []).append(k)
    return by


def _panel(c2, **env):
    """Both + its CompiledPanel, created under the given switches (a panel reads them once, when it is created)."""
    from specimux_amd.demultiplex import compiled_panel
    _pan, (pf, sf) = c2
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        both = Both(pf, sf)
        return both, compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def tile_panel(lib, c2):
    return _panel(c2)


@pytest.fixture(scope="module")
def planes_panel(lib, c2):
    return _panel(c2, SMX_PRESCAN_PLANES="1")


def _raw(both, cp, reads):
    from specimux_amd.demultiplex import concat_records
    from specimux_amd.io_utils import SeqRecord
    bases, offsets, _ = concat_records([SeqRecord(s, rid, rid, q) for rid, s, q in reads])
    windows, lens = cp.pack_windows(bases, offsets)
    ops, extra, counts, hits, _bd = cp.run(windows, lens, want_hits="lean")
    return ops, np.sort(extra, order=EXTRA_ORDER), counts, hits


def _hit_sample(reads):
    n = len(reads)
    idx = sorted({i for i in list(range(10)) + list(range(250, 260)) + list(range(1018, 1030)) + list(range(n - 10, n)) if 0 <= i < n})
    return [reads[i] for i in idx]


def _check(both, cp, planes, reads, oracle, label):
    """the tile-codes panel `cp` on `reads`: against the oracle, and against the planes panel"""
    got, _total, _matched = both.product_ops(reads)
    by = {}
    for k in got:
        by.setdefault(k[0], []).append(k)
    for rid, _s, _q in reads:
        assert by.get(rid) == oracle.get(rid), f"{label}: read {rid}: gpu {by.get(rid)} oracle {oracle.get(rid)}"
    both.assert_hits_equal(_hit_sample(reads), label, lean=True)
    a, b = _raw(both, cp, reads), _raw(planes[0], planes[1], reads)
    assert np.array_equal(a[0], b[0]), f"{label}: records differ from the planes path"
    assert np.array_equal(a[1], b[1]), f"{label}: extra records differ from the planes path"
    assert np.array_equal(a[2], b[2]), f"{label}: counts differ from the planes path"
    for f in HIT_FIELDS:
        assert np.array_equal(a[3][f], b[3][f]), f"{label}: hit dump field {f} differs from the planes path"


def test_default_is_tile_codes_and_switch_gives_planes(lib, c2, reads, capfd):
    """SMX_DEBUG names the text source of the DP kernel when a panel first touches the device."""
    for env, word in ((dict(SMX_DEBUG="1"), "prescan (tile codes)"), (dict(SMX_DEBUG="1", SMX_PRESCAN_PLANES="1"), "prescan (planes)")):
        both, cp = _panel(c2, **env)
        capfd.readouterr()
        _raw(both, cp, reads[:33])
        assert word in capfd.readouterr().err


@pytest.mark.parametrize("n", READ_COUNTS)
def test_read_counts(tile_panel, planes_panel, reads, oracle, n):
    _check(*tile_panel, planes_panel, reads[:n], oracle, f"tile codes n={n}")


@pytest.mark.parametrize("n", [257, 2049])
def test_generic_demux_kernel(lib, c2, reads, oracle, n):
    """SMX_NO_SPECIALISE: the generic instantiation's encode reads the same tile-major buffer"""
    both, cp = _panel(c2, SMX_NO_SPECIALISE="1")
    _check(both, cp, _panel(c2, SMX_NO_SPECIALISE="1", SMX_PRESCAN_PLANES="1"), reads[:n], oracle, f"generic n={n}")


def test_demux_tile_that_does_not_divide_the_dp_tile(lib, c2, reads, oracle):
    """48-read demux tiles: tile 21 holds reads 1008 .. 1055, on both sides of the first DP tile's edge"""
    both, cp = _panel(c2, SMX_TILE_R="48")
    _check(both, cp, _panel(c2, SMX_TILE_R="48", SMX_PRESCAN_PLANES="1"), reads, oracle, "48-read tiles")


def test_two_batches_in_flight(lib, tile_panel, planes_panel, reads, oracle):
    """two batches on two streams, each with its own code buffer: every batch equals the same batch run alone, which in turn
    equals the oracle and the planes path (the first batch through test_read_counts[2049], the second here)"""
    import torch
    from specimux_amd import _lib
    from specimux_amd.demultiplex import concat_records
    from specimux_amd.io_utils import SeqRecord
    _both, cp = tile_panel
    _check(*tile_panel, planes_panel, reads[::-1][:1025], oracle, "second batch")
    dev = torch.device("cuda", 0)
    sets, alone = [], []
    for batch in (reads, reads[::-1][:1025]):
        bases, offsets, _ = concat_records([SeqRecord(s, rid, rid, q) for rid, s, q in batch])
        w, l = cp.pack_windows(bases, offsets)
        ops, extra, counts = cp.run(w, l)
        sets.append((w, l))
        alone.append((ops.copy(), np.sort(extra, order=EXTRA_ORDER), counts.copy()))
    cp.set_streams(2)
    try:
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        bufs = []
        for w, l in sets:
            n = len(l)
            bufs.append(dict(n=n, w=torch.from_numpy(w).to(dev), l=torch.from_numpy(l).to(dev),
                             ops=torch.zeros(n * 32, dtype=torch.uint8, device=dev), extra=torch.zeros(n * 32, dtype=torch.uint8, device=dev),
                             ne=torch.zeros(4, dtype=torch.int32, device=dev), counts=torch.zeros(cp.counts_len, dtype=torch.int64, device=dev)))
        torch.cuda.synchronize()
        for _round in range(2):
            for k, b in enumerate(bufs):
                _lib.check(lib.smx_batch_run_device(cp.handle, C.c_void_p(streams[k].cuda_stream), C.c_void_p(b["w"].data_ptr()),
                                                    C.c_void_p(b["l"].data_ptr()), b["n"], C.c_void_p(b["ops"].data_ptr()),
                                                    C.c_void_p(b["extra"].data_ptr()), b["n"], C.c_void_p(b["ne"].data_ptr()),
                                                    C.c_void_p(b["counts"].data_ptr()), None, None))
        torch.cuda.synchronize()
        for k, b in enumerate(bufs):
            ne = int(b["ne"][0].item())
            assert np.array_equal(b["ops"].cpu().numpy().view(_lib.OP_DTYPE), alone[k][0]), k
            assert np.array_equal(np.sort(b["extra"].cpu().numpy().view(_lib.OP_DTYPE)[:ne], order=EXTRA_ORDER), alone[k][1]), k
            assert np.array_equal(b["counts"].cpu().numpy().astype(np.uint64), 2 * alone[k][2]), k
    finally:
        cp.set_streams(1)
