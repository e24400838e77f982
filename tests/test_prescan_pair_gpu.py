"""The primer DP kernel (prescan_dp_kernel, smx_prescan.hip) on the GPU at the batch sizes and panels where its column
bookkeeping, its work-item mapping or its per-wave scratch can go wrong: records and hit tables against the CPU oracle,
through the helpers of test_gpu_parity.py."""
import ctypes as C

import pytest

from parity_utils import Both, reads_from_set, tmp_panel

pytestmark = pytest.mark.gpu


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
    return pan, tmp_panel(tmp_path_factory, pan, "c2")


@pytest.fixture(scope="module")
def c3(tmp_path_factory):
    from specimux_amd import synth
    pan = synth.panel_c3()
    return pan, tmp_panel(tmp_path_factory, pan, "c3")


@pytest.fixture(scope="module")
def c2_reads(c2):
    """One read set for every batch size: generated once, sliced by the tests."""
    from specimux_amd import synth
    rs = synth.make_reads(c2[0], 2049, 4242, windows_only=False)
    return reads_from_set(rs, range(2049), 80)


def _hit_sample(reads):
    """Reads whose hit tables are compared: both ends of the batch and the reads around the 1024-read tile edges."""
    n = len(reads)
    idx = sorted({i for i in list(range(12)) + list(range(1018, 1030)) + list(range(2042, 2049)) + list(range(n - 12, n))
                  if 0 <= i < n})
    return [reads[i] for i in idx]


# partial 32-read group, one group + 1, a tile less one read, a tile + 1 (two tiles), two tiles + 1 (three tiles: work items
# of several tiles and primers go through one wave's scratch buffers in turn)
@pytest.mark.parametrize("n", [1, 33, 1023, 1025, 2049])
def test_read_counts_two_primer_panel(lib, c2, c2_reads, n):
    _pan, (pf, sf) = c2
    both = Both(pf, sf)
    reads = c2_reads[:n]
    both.assert_hits_equal(_hit_sample(reads), f"c2 n={n}", lean=True)
    both.assert_ops_equal(reads, f"c2 n={n}")


def test_two_primer_panel_one_chunk_window(lib, c2):
    """search_len 16: one 16-column chunk, the shortest window the DP kernel serves."""
    from specimux_amd import synth
    pan, (pf, sf) = c2
    rs = synth.make_reads(pan, 300, 1616, search_len=16, windows_only=False)
    reads = reads_from_set(rs, range(300), 16)
    both = Both(pf, sf, search_len=16)
    both.assert_hits_equal(reads[:60], "c2 S=16")
    both.assert_ops_equal(reads, "c2 S=16")


@pytest.mark.parametrize("search_len", [80, 160])
def test_eight_primer_panel(lib, c3, search_len):
    """Degenerate primers at p = 2, 3, 6, 7: every primer must read its own letter sets (and the match words: this panel
    runs the compact demux tiles)."""
    from specimux_amd import synth
    pan, (pf, sf) = c3
    kw = dict(search_len=160, error_rate=0.15) if search_len == 160 else dict(insert_mean=900, insert_sd=250)
    rs = synth.make_reads(pan, 400, 3300 + search_len, windows_only=False, **kw)
    reads = reads_from_set(rs, range(400), search_len)
    both = Both(pf, sf, **(dict(search_len=160) if search_len == 160 else {}))
    both.assert_hits_equal(reads[:60], f"c3 S={search_len}")
    got = both.assert_ops_equal(reads, f"c3 S={search_len}")
    assert sum(1 for k in got if k[6] == "DEREP") > 50


def test_31nt_primer_every_row_live(lib, tmp_path_factory):
    from specimux_amd import synth
    f, r = synth.make_barcodes(8, 6, length=13, min_dist=6, seed=7)
    pan = synth.Panel([("ITS", "FWD", "CTTGGTCATTTAGAGGAAGTAAAAGTCGTAA", "ITS4", synth.ITS4)], f, r)
    pf, sf = tmp_panel(tmp_path_factory, pan, "p31")
    rs = synth.make_reads(pan, 400, 3131, windows_only=False)
    reads = reads_from_set(rs, range(400), 80)
    both = Both(pf, sf)
    both.assert_hits_equal(reads[:60], "31nt primer")
    got = both.assert_ops_equal(reads, "31nt primer")
    assert sum(1 for k in got if k[6] == "DEREP") > 100
