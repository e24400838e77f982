"""The per-specimen counters of the demux kernel and the launch counters its last workgroup re-arms (the kernel's epilogue,
workgroup_done: the extra-record count is published, the tile queue, the finished-workgroup count and the overflow list are
zeroed for the next launch).

Every case: counts[CNT_SPECIMEN0:] of a launch equals a host histogram of that launch's own records (the primary record of
every read that has one, plus the extra records; class full -- not UNKNOWN, not PARTIAL_FWD / PARTIAL_REV -- and a specimen),
and the records of a sample of reads tally to what the oracle's records of those reads tally to.  The shapes are the sizes
at which the counting and the re-arming can go wrong: no read, one read (nearly every workgroup leaves without a tile, and
a second launch right behind must find the counters re-armed), a partial tile, one full tile, a tile and one read, five
tiles, 79 tiles; the generic instantiation; a compact launch whose redo launch has work (the
chain re-arms once, in the redo launch); reads with several records; several launches into one counts vector on one stream
and on three.  (run on the MI355X box: `pytest -m gpu`)"""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from oracle import specimux_oracle as O
from parity_utils import Both, reads_from_set, tmp_panel

pytestmark = pytest.mark.gpu

N_ORACLE = 48   # reads of a batch whose records are also tallied against the oracle's


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


_READS = {}


def reads_of(which, pan, n, seed, **kw):
    """A generated read set, made once per module and left unchanged."""
    from specimux_amd import synth
    key = (which, n, seed, tuple(sorted(kw.items())))
    if key not in _READS:
        _READS[key] = synth.make_reads(pan, n, seed, **kw)
    return _READS[key]


def panel_for(files, **flags):
    """(Both, CompiledPanel): a fresh panel, so that the environment switches of the moment apply."""
    from specimux_amd.demultiplex import compiled_panel
    both = Both(*files, **flags)
    return both, compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)


def histogram(ops, extra, n_specimens):
    """Per-specimen tally of a launch's own records, filtered as the kernel counts them."""
    from specimux_amd import _lib
    recs = np.concatenate([ops[ops["n_ops"] >= 1], extra])
    partial_or_unknown = np.isin(recs["rtype"], (_lib.R_UNKNOWN, _lib.R_PARTIAL_FWD, _lib.R_PARTIAL_REV))
    keep = ~partial_or_unknown & (recs["sample"] >= 0)
    return np.bincount(recs["sample"][keep], minlength=n_specimens).astype(np.uint64)


def specimen_counts(cp, counts):
    from specimux_amd import _lib
    return np.asarray(counts[_lib.CNT_SPECIMEN0:], dtype=np.uint64)


def check_against_oracle(both, cp, rs, ops, extra, label):
    """The records of the first N_ORACLE reads tally per specimen to what the oracle's records of those reads tally to."""
    n = min(N_ORACLE, len(ops))
    if n == 0:
        return
    reads = reads_from_set(rs, range(n), both.args.search_len)
    oops, _t, _m = O.process_sequences(reads, both.opar, both.opanel)
    exp = Counter(op.sample_id for op in oops if op.rtype in (O.R_FULL, O.R_MULTI, O.R_DEREP))
    got = histogram(ops[:n], extra[extra["read"] < n], len(cp.specimen_ids))
    assert {cp.specimen_ids[i]: int(c) for i, c in enumerate(got) if c} == dict(exp), label


def run_and_check(both, cp, rs, label, oracle=True, n=None):
    """n: run the first n reads of the set only."""
    windows, lens = rs.windows(cp.window_stride), rs.lens
    if n is not None:
        windows, lens = windows[:n], lens[:n]
    ops, extra, counts = cp.run(windows, lens)
    hist = histogram(ops, extra, len(cp.specimen_ids))
    got = specimen_counts(cp, counts)
    print(f"{label}: {len(lens)} reads, {len(extra)} extra records, {int(hist.sum())} counted, {int((hist > 0).sum())} specimens")
    assert np.array_equal(got, hist), f"{label}: {int(got.sum())} counted by the kernel, {int(hist.sum())} in its records"
    if oracle:
        check_against_oracle(both, cp, rs, ops, extra, label)
    return ops, extra, got


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_counts_equal_the_launchs_records(lib, c2, n):
    pan, files = c2
    both, cp = panel_for(files)
    rs = reads_of("c2", pan, max(n, 1), 7100 + n)      # (no reads: the first 0 of a set of one)
    _ops, _extra, first = run_and_check(both, cp, rs, f"c2 n={n}", n=n)
    if n == 0:
        assert first.sum() == 0
    if n == 5000:
        assert first.sum() > 3000 and (first > 0).sum() > 500      # counted across the panel
    if n == 1:
        # nearly every workgroup of that launch found the queue empty; whichever came last had to re-arm the launch
        # counters: a second launch right behind it scores and counts the same read once
        _ops, _extra, second = run_and_check(both, cp, rs, "c2 n=1 again", oracle=False)
        assert np.array_equal(first, second)


def test_generic_instantiation(lib, c2, monkeypatch):
    monkeypatch.setenv("SMX_NO_SPECIALISE", "1")
    pan, files = c2
    both, cp = panel_for(files)
    run_and_check(both, cp, reads_of("c2", pan, 5000, 7100 + 5000), "c2 generic")


def test_compact_and_redo_chain(lib, c3, monkeypatch):
    """SMX_COMPACT_ITEMS=16: compact tiles of 16 records overflow, so the dense redo launch behind the compact one has reads
    of its own to count; only the redo launch, the chain's last, publishes the extra-record count and re-arms the rest."""
    monkeypatch.setenv("SMX_COMPACT_ITEMS", "16")
    pan, files = c3
    both, cp = panel_for(files)
    rs = reads_of("c3", pan, 5000, 7203)
    _ops, _extra, first = run_and_check(both, cp, rs, "c3 compact + redo")
    assert first.sum() > 3000
    _ops, _extra, second = run_and_check(both, cp, rs, "c3 compact + redo again", oracle=False)
    assert np.array_equal(first, second)


def test_reads_with_several_records(lib, c3):
    """Barcode ties: with --dereplicate none, index distance 4 and no prefilter many reads resolve to several specimens, one
    record each, every one of them counted."""
    from specimux_amd import _lib
    pan, files = c3
    both, cp = panel_for(files, dereplicate="none", index_edit_distance=4, disable_prefilter=True)
    rs = reads_of("c3", pan, 4096, 4242, insert_mean=900, insert_sd=250)
    ops, extra, _got = run_and_check(both, cp, rs, "c3 ties")
    assert ops["n_ops"].max() > 1
    counted_extra = ~np.isin(extra["rtype"], (_lib.R_UNKNOWN, _lib.R_PARTIAL_FWD, _lib.R_PARTIAL_REV)) & (extra["sample"] >= 0)
    assert counted_extra.sum() >= 8, "the batch was built to have extra records that name a specimen"


def _device_launches(lib, cp, sets, plan):
    """plan: (stream index, read set index) per launch, all into one counts vector.  -> (counts, per-launch histograms)"""
    import torch
    from specimux_amd import _lib
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream() for _ in range(1 + max(s for s, _ in plan))]
    counts = torch.zeros(cp.counts_len, dtype=torch.int64, device=dev)
    bufs = []
    for _s, k in plan:
        rs = sets[k]
        n = len(rs.lens)
        bufs.append(dict(n=n, w=torch.from_numpy(rs.windows(cp.window_stride)).to(dev), l=torch.from_numpy(rs.lens).to(dev),
                         ops=torch.zeros(n * 32, dtype=torch.uint8, device=dev), extra=torch.zeros(n * 32, dtype=torch.uint8, device=dev),
                         ne=torch.zeros(4, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    for (s, _k), b in zip(plan, bufs):
        _lib.check(lib.smx_batch_run_device(cp.handle, C.c_void_p(streams[s].cuda_stream), C.c_void_p(b["w"].data_ptr()),
                                            C.c_void_p(b["l"].data_ptr()), b["n"], C.c_void_p(b["ops"].data_ptr()),
                                            C.c_void_p(b["extra"].data_ptr()), b["n"], C.c_void_p(b["ne"].data_ptr()),
                                            C.c_void_p(counts.data_ptr()), None, None))
    torch.cuda.synchronize()
    hists = []
    for b in bufs:
        ne = int(b["ne"][0].item())
        assert ne <= b["n"]
        hists.append(histogram(b["ops"].cpu().numpy().view(_lib.OP_DTYPE), b["extra"].cpu().numpy().view(_lib.OP_DTYPE)[:ne],
                               len(cp.specimen_ids)))
    return specimen_counts(cp, counts.cpu().numpy().astype(np.uint64)), hists


def test_launches_into_one_counts_vector(lib, c2):
    """Three launches on one stream, then two on each of three streams (smx_panel_set_streams(3): each stream has its own
    launch counters, all add into the same counts): the total is the sum of the launches' own histograms."""
    pan, files = c2
    _both, cp = panel_for(files)
    sets = [reads_of("c2", pan, n, 7300 + n) for n in (5000, 3001, 257)]
    got, hists = _device_launches(lib, cp, sets, [(0, 0), (0, 1), (0, 2)])
    assert all(h.sum() > 100 for h in hists)
    assert np.array_equal(got, sum(hists)), "three launches on one stream"
    cp.set_streams(3)
    try:
        got, hists = _device_launches(lib, cp, sets, [(0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (2, 0)])
        assert np.array_equal(got, sum(hists)), "two launches on each of three streams"
    finally:
        cp.set_streams(1)
