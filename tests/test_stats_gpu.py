"""specimux-stats on the GPU: the table the statistics kernel accumulates from the demux kernel's lean hit dump and primary
records equals, key for key and count for count, the table the host aggregator builds from the oracle's trace of the same
reads; accumulation over batches and streams; `--from-run` end to end against the reference's committed output."""
import ctypes as C
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import specimux_oracle as O
from parity_utils import FUZZ_FLAG_SETS, Both, reads_from_set, tmp_panel
from stats_utils import REPO, STATS_GOLDEN, oracle_table

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(REPO, "tests", "golden", "integration_test_suite")
P, S = f"{GOLDEN}/primers.fasta", f"{GOLDEN}/specimens.txt"
GEN_KNOBS = ("error_rate", "n_frac")     # knobs of the read generator inside FUZZ_FLAG_SETS, not specimux flags


@pytest.fixture(scope="module")
def lib():
    from specimux_amd import _lib
    lib = _lib.load()
    n = C.c_int(0)
    _lib.check(lib.smx_device_init(0, C.byref(n)))
    assert n.value >= 1
    return lib


@pytest.fixture(scope="module")
def panels(tmp_path_factory):
    from specimux_amd import synth
    out = {}
    for name, pan in (("c1", synth.panel_c1()), ("c2", synth.panel_c2()), ("c3", synth.panel_c3())):
        out[name] = (pan, tmp_panel(tmp_path_factory, pan, "stats_" + name))
    return out


def windows_of(cp, reads):
    from specimux_amd.demultiplex import concat_records
    from specimux_amd.io_utils import SeqRecord
    bases, offsets, seqs = concat_records([SeqRecord(s, rid, rid, q) for rid, s, q in reads])
    windows, lens = cp.pack_windows(bases, offsets)
    return windows, lens, seqs


def device_table(both, batches, capacity=1 << 15, n_slots=2, extra_cap=None):
    """Stats table of window batches [(windows, lens, seqs or None)] counted on the device -> (table, counts vector)."""
    from specimux_amd import trace_stats
    from specimux_amd.demultiplex import compiled_panel
    cp = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
    stats = trace_stats.DeviceStats(cp, capacity)
    try:
        replay = trace_stats.HostReplay(cp, both.parameters, both.specimens, both.args, both.prefilter is not None)
        table = trace_stats.StatsTable()
        counts = trace_stats.accumulate_batches(cp, stats, batches, replay, table, n_slots=n_slots, extra_cap=extra_cap)
        keys, cnts = stats.read()
    finally:
        stats.close()
    return trace_stats.table_from_keys(cp, keys, cnts, table), counts


def assert_parity(both, reads, label):
    from specimux_amd.demultiplex import compiled_panel
    cp = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
    got, counts = device_table(both, [windows_of(cp, reads)])
    exp, rows = oracle_table(both.opanel, both.opar, reads)
    if got != exp:
        diff = {k: (got.counts.get(k, 0), exp.counts.get(k, 0)) for k in set(got.counts) | set(exp.counts)
                if got.counts.get(k, 0) != exp.counts.get(k, 0)}
        raise AssertionError(f"{label}: {len(diff)} row(s) differ (device, oracle trace): {list(diff.items())[:6]}")
    trim_empty = len({r[2] for r in rows if r[3] == "SEQUENCE_TRIM_EMPTY"})
    print(f"{label}: {len(reads)} reads, {len(exp.counts)} rows, host_replayed {got.host_replayed} of {trim_empty} trim-empty reads")
    assert got.host_replayed <= trim_empty, (label, got.host_replayed, trim_empty)
    assert got.total("sequences") == len(reads) == int(counts[0])
    return got


def _flags(fs):
    return {k: v for k, v in fs.items() if k not in GEN_KNOBS}


_FLAG_IDS = [",".join(f"{k}={v}" for k, v in fs.items()) or "default" for fs in FUZZ_FLAG_SETS]


@pytest.mark.parametrize("fs", FUZZ_FLAG_SETS, ids=_FLAG_IDS)
def test_table_parity_golden_and_edge_reads(lib, panels, fs):
    from test_gpu_parity import _edge_reads
    reads, _ = O.read_sequences(f"{GOLDEN}/sequences.fastq")
    rc, _ = O.read_sequences(f"{GOLDEN}/sequences_rc.fastq")
    assert_parity(Both(P, S, **_flags(fs)), reads + [("rc_" + i, s, q) for i, s, q in rc], f"golden {fs}")
    pan, (pf, sf) = panels["c2"]
    edge = [r for r in _edge_reads(pan) if r[0] != "u_base"]
    assert_parity(Both(pf, sf, **_flags(fs)), edge, f"edge {fs}")


@pytest.mark.parametrize("fs", FUZZ_FLAG_SETS, ids=_FLAG_IDS)
@pytest.mark.parametrize("which", ["c1", "c2", "c3"])
def test_table_parity_synthetic_reads(lib, panels, which, fs):
    from specimux_amd import synth
    pan, (pf, sf) = panels[which]
    S_ = fs.get("search_len", 80)
    gen = {k: fs[k] for k in GEN_KNOBS if k in fs}
    if which == "c3":
        gen.update(insert_mean=900, insert_sd=250)
    rs = synth.make_reads(pan, 1500, 7100 + len(which) + 17 * FUZZ_FLAG_SETS.index(fs), search_len=S_, windows_only=False, **gen)
    assert_parity(Both(pf, sf, **_flags(fs)), reads_from_set(rs, range(1500), S_), f"{which} {fs}")


def test_accumulation_over_batches_streams_and_small_extra_buffer(lib, panels):
    from specimux_amd import synth
    from specimux_amd.demultiplex import compiled_panel
    pan, (pf, sf) = panels["c3"]
    both = Both(pf, sf, dereplicate="none", index_edit_distance=4, disable_prefilter=True)   # many multi-record reads
    cp = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
    rs = synth.make_reads(pan, 6000, 424, windows_only=False, insert_mean=900, insert_sd=250)
    w, l, seqs = windows_of(cp, reads_from_set(rs, range(6000), 80))
    one, counts = device_table(both, [(w, l, seqs)])
    cut = [(w[a:b], l[a:b], seqs[a:b]) for a, b in ((0, 2500), (2500, 2501), (2501, 6000))]
    three, counts3 = device_table(both, cut, n_slots=2)
    tiny, counts_t = device_table(both, [(w, l, seqs)], extra_cap=1)
    assert one == three == tiny and one.total("sequences") == 6000
    assert np.array_equal(counts, counts3) and np.array_equal(counts, counts_t)
    from specimux_amd import _lib
    assert counts[_lib.CNT_MULTI_OP_READS] > 1     # the one-record extra buffer did overflow
    assert one.host_replayed == three.host_replayed == tiny.host_replayed


def _from_run(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, "-m", "specimux_amd.trace_stats", "--from-run"] + args, cwd=REPO, env=env,
                          capture_output=True, text=True, timeout=timeout)


def _fixture(case, name):
    return open(os.path.join(STATS_GOLDEN, case, name + ".txt"), encoding="utf-8").read()


def test_from_run_prints_the_reference_output(lib, tmp_path):
    gz = tmp_path / "sequences.fastq.gz"
    with open(f"{GOLDEN}/sequences.fastq", "rb") as src, gzip.open(gz, "wb") as dst:
        shutil.copyfileobj(src, dst)
    lists = (("hier_pool_pair_detailed", ["--hierarchical", "pool", "primer_pair", "outcome_detailed"]),
             ("hier_orientation_by_sequences", ["--hierarchical", "orientation", "match_type", "resolution_type", "--count-by", "sequences"]))
    for seqfile in (f"{GOLDEN}/sequences.fastq", os.fspath(gz)):
        for name, dims in lists:
            res = _from_run([P, S, seqfile] + dims)
            assert res.returncode == 0, res.stderr
            assert res.stdout == _fixture("golden_default", name), (seqfile, name)
            assert "host_replayed" in res.stderr
    for name, dims in lists:
        res = _from_run([P, S, f"{GOLDEN}/sequences.fastq", "-n", "11,20"] + dims)
        assert res.returncode == 0, res.stderr
        assert res.stdout == _fixture("golden_n11_20", name), name
    for case, flags in (("golden_derep_none", ["--dereplicate", "none"]), ("golden_no_preorient", ["--disable-preorient"]),
                        ("golden_min_length_600", ["--min-length", "600"])):
        res = _from_run([P, S, f"{GOLDEN}/sequences.fastq"] + flags + lists[0][1])
        assert res.returncode == 0, res.stderr
        assert res.stdout == _fixture(case, lists[0][0]), case


def test_from_run_save_table_then_query(lib, tmp_path, capsys):
    from specimux_amd import cli
    saved = tmp_path / "run.json"
    res = _from_run([P, S, f"{GOLDEN}/sequences.fastq", "--save-table", os.fspath(saved), "--list-dimensions"])
    assert res.returncode == 0, res.stderr
    assert res.stdout == _fixture("golden_default", "dimensions")
    assert cli.trace_main(["--table", os.fspath(saved), "--hierarchical", "forward_barcode_matched", "barcode_count", "outcome"]) == 0
    assert capsys.readouterr().out == _fixture("golden_default", "hier_barcodes_outcome")


def test_full_table_is_loud(lib, panels, tmp_path):
    from specimux_amd import synth
    pan, (pf, sf) = panels["c2"]
    fq = tmp_path / "c2.fastq"
    synth.make_reads(pan, 1500, 2002, windows_only=False).write_fastq(os.fspath(fq))
    res = _from_run([pf, sf, os.fspath(fq), "--table-capacity", "8", "--hierarchical", "pool", "outcome"])
    assert res.returncode == 1 and res.stdout == ""
    assert "libsmx error -4" in res.stderr and "--table-capacity" in res.stderr and "full" in res.stderr
    ok = _from_run([pf, sf, os.fspath(fq), "--hierarchical", "pool", "outcome"])
    assert ok.returncode == 0 and ok.stdout.startswith("Hierarchical Statistics: pool → outcome\nCount by: candidate_matches\n")


def test_bench_workload_765k(lib, panels):
    """The benchmark's workload: totals, independence of the batch size, and the first 2 000 reads against the oracle."""
    from specimux_amd import _lib, synth
    from specimux_amd.demultiplex import compiled_panel
    pan, (pf, sf) = panels["c2"]
    both = Both(pf, sf)
    cp = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
    n = 765000
    rs = synth.make_reads(pan, n, 2002)
    w = rs.windows(cp.window_stride)

    def cut(size):
        return [(w[a:a + size], rs.lens[a:a + size], None) for a in range(0, n, size)]
    whole, counts = device_table(both, cut(n), capacity=1 << 16)
    parts, counts_p = device_table(both, cut(200_000), capacity=1 << 16, n_slots=3)
    assert whole == parts and np.array_equal(counts, counts_p)
    assert whole.total("sequences") == n == int(counts[_lib.CNT_TOTAL])
    assert whole.host_replayed == parts.host_replayed
    print(f"765k reads: {len(whole.counts)} rows, {whole.total()} candidates, host_replayed {whole.host_replayed}")
    head = reads_from_set(rs, range(2000), 80)
    first, _c = device_table(both, [(w[:2000], rs.lens[:2000], None)])
    exp, _rows = oracle_table(both.opanel, both.opar, head)
    assert first == exp
