"""`--stats-table` on the GPU: an ordinary `-F` run leaves its stats table beside its tree (one GPU, two ranks), the
watcher keeps one cumulative table.  Yardsticks: what the reference's tool printed for the reference's traces
(tests/golden/stats/) and the table the host aggregator builds from the oracle's trace of the same reads
(stats_utils.oracle_table) -- never a table the code under test produced by another route."""
import ctypes as C
import functools
import gzip
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import specimux_oracle as O
from parity_utils import Both
from stats_utils import REPO, STATS_GOLDEN, oracle_table, queries_of
from test_watch_gpu import GOLDEN_CUTS, Watch, split_fastq, tree_bytes

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(REPO, "tests", "golden", "integration_test_suite")
P, S = f"{GOLDEN}/primers.fasta", f"{GOLDEN}/specimens.txt"
SEED = 8101      # c2: 2, c3: 11 reads of the 3 000 are SEQUENCE_TRIM_EMPTY in the oracle's trace, under both flag sets below
FLAG_SETS = {"default": ([], {}),
             "derep_none_e4_noprefilter": (["--dereplicate", "none", "-e", "4", "--disable-prefilter"],
                                           dict(dereplicate="none", index_edit_distance=4, disable_prefilter=True))}


@pytest.fixture(scope="module")
def lib():
    from specimux_amd import _lib
    lib = _lib.load()
    n = C.c_int(0)
    _lib.check(lib.smx_device_init(0, C.byref(n)))
    assert n.value >= 1
    return lib


@pytest.fixture(autouse=True)
def _restore_env(monkeypatch):
    # the watcher sets these for its process: undo that after each test
    for name in ("SMX_IO_NO_MMAP", "SMX_IO_THREADS"):
        if name in os.environ:
            monkeypatch.setenv(name, os.environ[name])
        else:
            monkeypatch.setenv(name, "x")
            monkeypatch.delenv(name)
    yield


@pytest.fixture(scope="module")
def synth_files(tmp_path_factory):
    """{c2, c3: (primer file, specimen file, FASTQ of 3 000 reads)}"""
    from specimux_amd import synth
    out = {}
    for which, pan, gen in (("c2", synth.panel_c2(), {}), ("c3", synth.panel_c3(), dict(insert_mean=900, insert_sd=250))):
        d = tmp_path_factory.mktemp("runstats_" + which)
        pf, sf = pan.write(os.fspath(d))
        fq = os.path.join(os.fspath(d), "reads.fastq")
        synth.make_reads(pan, 3000, SEED, windows_only=False, **gen).write_fastq(fq)
        out[which] = (pf, sf, fq)
    return out


@functools.lru_cache(maxsize=None)
def oracle_of(pf, sf, fq, flag_set):
    """(oracle's table of the file's reads, number of reads, number of SEQUENCE_TRIM_EMPTY reads)"""
    both = Both(pf, sf, **FLAG_SETS[flag_set][1])
    reads, _ = O.read_sequences(fq)
    table, rows = oracle_table(both.opanel, both.opar, reads)
    return table, len(reads), len({r[2] for r in rows if r[3] == "SEQUENCE_TRIM_EMPTY"})


def run_cli(argv, env=None, check=True):
    """`python -m specimux_amd.cli` in a process of its own (environment hooks are read at import)."""
    res = subprocess.run([sys.executable, "-m", "specimux_amd.cli"] + [os.fspath(a) for a in argv], cwd=REPO,
                         env=dict(os.environ, PYTHONPATH=REPO, **(env or {})), capture_output=True, text=True, timeout=600)
    if check:
        assert res.returncode == 0, res.stderr[-3000:]
    return res


def load(path):
    from specimux_amd.trace_stats import StatsTable
    return StatsTable.load(path)


def assert_tables_equal(got, exp, label):
    if got != exp:
        diff = {k: (got.counts.get(k, 0), exp.counts.get(k, 0)) for k in set(got.counts) | set(exp.counts)
                if got.counts.get(k, 0) != exp.counts.get(k, 0)}
        raise AssertionError(f"{label}: {len(diff)} row(s) differ (run, yardstick): {list(diff.items())[:6]}")


def processed_reads(out_dir):
    """CNT_TOTAL of the run, from its summary line."""
    m = re.search(r"Processed ([\d,]+) sequences", open(os.path.join(out_dir, "log.txt")).read())
    return int(m.group(1).replace(",", ""))


def assert_prints_the_fixtures(table_path, case, tmp_path, capsys):
    from specimux_amd import cli
    for q in queries_of(case):
        if q["kind"] == "sankey":
            out = tmp_path / (q["name"] + ".json")
            assert cli.trace_main(["--table", os.fspath(table_path)] + q["args"] + ["--output", os.fspath(out)]) == 0
            got = json.load(open(out))
            exp = json.load(open(os.path.join(STATS_GOLDEN, case, q["name"] + ".json")))
            exp["links"].sort(key=lambda link: (link["source"], link["target"]))   # as tests/test_stats_cpu.py: link order
            assert got == exp and list(got) == list(exp), (case, q["name"])
            capsys.readouterr()
        else:
            assert cli.trace_main(["--table", os.fspath(table_path)] + q["args"]) == 0
            text = capsys.readouterr().out
            assert text == open(os.path.join(STATS_GOLDEN, case, q["name"] + ".txt"), encoding="utf-8").read(), (case, q["name"])


# ------------------------------------------------------------------ 1, 2: the reference's committed output
@pytest.mark.parametrize("case,flags", [("golden_default", []), ("golden_n11_20", ["-n", "11,20"]),
                                        ("golden_derep_none", ["--dereplicate", "none"]),
                                        ("golden_no_preorient", ["--disable-preorient"]),
                                        ("golden_min_length_600", ["--min-length", "600"])])
def test_run_table_prints_the_reference_output(lib, tmp_path, capsys, case, flags):
    from specimux_amd import cli
    gz = tmp_path / "sequences.fastq.gz"
    with open(f"{GOLDEN}/sequences.fastq", "rb") as src, gzip.open(gz, "wb") as dst:
        shutil.copyfileobj(src, dst)
    for n, seqfile in enumerate((f"{GOLDEN}/sequences.fastq", os.fspath(gz))):
        table = tmp_path / f"t{n}.json"
        cli.main(["specimux", P, S, seqfile, "-F", "-O", str(tmp_path / f"out{n}"), "--stats-table", str(table)] + flags)
        log = (tmp_path / f"out{n}" / "log.txt").read_text()
        assert f"Stats table {table}" in log and "host_replayed" in log and "distinct rows" in log
        capsys.readouterr()
        assert_prints_the_fixtures(table, case, tmp_path, capsys)


# ------------------------------------------------------------------ 3: the tree does not depend on the flag
def test_tree_is_identical_with_and_without_the_flag(lib, tmp_path, synth_files):
    from specimux_amd import cli
    pf, sf, fq = synth_files["c3"]
    for label, (primers, specimens, seqfile) in (("golden", (P, S, f"{GOLDEN}/sequences.fastq")), ("c3", (pf, sf, fq))):
        plain, counted = tmp_path / f"{label}_plain", tmp_path / f"{label}_counted"
        cli.main(["specimux", primers, specimens, seqfile, "-F", "-O", str(plain)])
        cli.main(["specimux", primers, specimens, seqfile, "-F", "-O", str(counted), "--stats-table", str(tmp_path / f"{label}.json")])
        a, b = tree_bytes(plain), tree_bytes(counted)
        assert a == b and sum(1 for v in a.values() if v) > 5, label
        assert (tmp_path / f"{label}.json").exists()


# ------------------------------------------------------------------ 4: oracle parity through reused lanes
@pytest.mark.parametrize("flag_set", list(FLAG_SETS))
@pytest.mark.parametrize("which", ["c2", "c3"])
def test_table_through_the_lanes_equals_the_oracle(lib, tmp_path, synth_files, which, flag_set):
    pf, sf, fq = synth_files[which]
    exp, n_reads, trim_empty = oracle_of(pf, sf, fq, flag_set)
    assert n_reads == 3000 and trim_empty >= 1      # the fallback list has work to do
    table = tmp_path / "t.json"
    # 1024 reads per batch: three batches, so every lane is used again after its first batch
    run_cli([pf, sf, fq, "-F", "-O", tmp_path / "out", "--stats-table", table] + FLAG_SETS[flag_set][0],
            env={"SMX_BATCH_READS": "1024"})
    got = load(table)
    print(f"{which} {flag_set}: {len(exp.counts)} rows, host_replayed {got.host_replayed} of {trim_empty} trim-empty reads")
    assert_tables_equal(got, exp, f"{which} {flag_set}")
    assert got.host_replayed <= trim_empty
    assert got.total("sequences") == processed_reads(tmp_path / "out") == n_reads


# ------------------------------------------------------------------ 5: both transport formats of the lanes
def test_ascii_and_4bit_lanes_agree(lib, tmp_path, synth_files):
    pf, sf, fq = synth_files["c3"]
    exp, _n, _te = oracle_of(pf, sf, fq, "default")
    tables = []
    for name, env in (("packed", {}), ("ascii", {"SMX_LANES_ASCII": "1"})):
        run_cli([pf, sf, fq, "-F", "-O", tmp_path / name, "--stats-table", tmp_path / f"{name}.json"],
                env=dict(env, SMX_BATCH_READS="1024"))
        tables.append(load(tmp_path / f"{name}.json"))
    assert_tables_equal(tables[1], tables[0], "ascii lanes against 4-bit lanes")
    assert_tables_equal(tables[1], exp, "ascii lanes against the oracle")
    assert tables[0].host_replayed == tables[1].host_replayed
    assert tree_bytes(tmp_path / "packed") == tree_bytes(tmp_path / "ascii")


# ------------------------------------------------------------------ 6: the lane ABI
def test_lane_abi(lib, tmp_path, synth_files):
    from specimux_amd import _lib, trace_stats
    from specimux_amd.demultiplex import compiled_panel, concat_records
    from specimux_amd.io_utils import SeqRecord
    from specimux_amd.native_io import Lane
    pf, sf, fq = synth_files["c2"]
    exp, _n, trim_empty = oracle_of(pf, sf, fq, "default")
    both = Both(pf, sf)
    cp = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
    reads, _ = O.read_sequences(fq)
    bases, offsets, seqs = concat_records([SeqRecord(s, rid, rid, q) for rid, s, q in reads])
    windows, lens = cp.pack_windows(bases, offsets)
    stats = trace_stats.DeviceStats(cp, 1 << 15)
    replay = trace_stats.HostReplay(cp, both.parameters, both.specimens, both.args, both.prefilter is not None)
    table = trace_stats.StatsTable()
    counts = np.zeros(cp.counts_len, dtype=np.uint64)
    lanes = [Lane(cp, 2048), Lane(cp, 2048)]
    fallback_reads = []

    def submit(lane, a, b):
        lane.windows[:b - a] = windows[a:b]
        lane.lens[:b - a] = lens[a:b]
        lane.submit(b - a)

    def retire(lane, a, b):
        ops, _extra = lane.wait(counts)
        assert len(ops) == b - a
        idx = np.sort(lane.fallback().astype(np.int64)) + a
        flagged = a + np.nonzero(ops["flags"] & _lib.OPF_TRIM_EMPTY)[0]
        assert idx.tolist() == flagged.tolist()      # the list is the reads whose primary record carries the flag
        if len(idx):
            replay.add_rows(table, windows[idx], lens[idx], [seqs[i] for i in idx])
        fallback_reads.extend(idx.tolist())

    try:
        with pytest.raises(_lib.SmxError) as e:      # nothing counted was retired on this lane yet
            lanes[0].fallback()
        assert e.value.code == _lib.ERR_ARG
        for ln in lanes:
            ln.attach_stats(stats)
        cuts = [(0, 1200), (1200, 1201), (1201, 3000)]     # three batches over two lanes, one of a single read
        submit(lanes[0], *cuts[0])
        submit(lanes[1], *cuts[1])
        retire(lanes[0], *cuts[0])
        submit(lanes[0], *cuts[2])
        retire(lanes[1], *cuts[1])
        retire(lanes[0], *cuts[2])
        # the oracle's own list of such reads: the first write operation is the unknown/unknown fallback of a candidate
        # that had matched a primer (stats_utils.sim_input marks the same reads for the CPU simulation)
        prefilter = O.make_prefilter(both.opanel, both.opar)
        want = []
        for i, rec in enumerate(reads):
            first = O.process_sequences([rec], both.opar, both.opanel, prefilter)[0][0]
            if (first.p1 == "unknown" and first.p1_loc is not None) or (first.p2 == "unknown" and first.p2_loc is not None):
                want.append(i)
        assert sorted(fallback_reads) == want and 1 <= len(want) <= trim_empty
        keys, cnts = stats.read()
        got = trace_stats.table_from_keys(cp, keys, cnts, table)
        assert_tables_equal(got, exp, "three batches over two lanes")
        assert got.total("sequences") == 3000 == int(counts[_lib.CNT_TOTAL])

        # detached: a further batch adds nothing
        for ln in lanes:
            ln.attach_stats(None)
        submit(lanes[0], 0, 1200)
        lanes[0].wait(counts)
        with pytest.raises(_lib.SmxError) as e:
            lanes[0].fallback()
        assert e.value.code == _lib.ERR_ARG
        keys2, cnts2 = stats.read()
        assert dict(zip(keys2.tolist(), cnts2.tolist())) == dict(zip(keys.tolist(), cnts.tolist()))

        # a table of another panel
        pf3, sf3, _fq3 = synth_files["c3"]
        other = Both(pf3, sf3)
        cp3 = compiled_panel(other.specimens, other.parameters, other.args, other.prefilter)
        stats3 = trace_stats.DeviceStats(cp3, 1 << 10)
        try:
            with pytest.raises(_lib.SmxError) as e:
                lanes[0].attach_stats(stats3)
            assert e.value.code == _lib.ERR_ARG and "another panel" in str(e.value)
        finally:
            stats3.close()

        # a lane with a batch in flight
        submit(lanes[1], 0, 100)
        with pytest.raises(_lib.SmxError) as e:
            lanes[1].attach_stats(stats)
        assert e.value.code == _lib.ERR_ARG and "in flight" in str(e.value)
        lanes[1].wait(counts)
        lanes[1].attach_stats(stats)       # and once it is retired the same call succeeds
        lanes[1].attach_stats(None)
    finally:
        for ln in lanes:
            ln.close()
        stats.close()


def test_lane_fallback_list_longer_than_what_travels_with_the_batch(lib, synth_files):
    """A lane sends the first 4 096 fallback indices with every batch and smx_lane_fallback fetches the rest: a lane of 8 192
    reads and one batch with more than 4 096 reads whose primary record trimmed to nothing (the c2 file's, tiled, between
    1 500 other rows of the file), then a small batch on the same lane, which must report its own short list."""
    import stats_utils as U
    from specimux_amd import _lib, trace_stats
    from specimux_amd.demultiplex import compiled_panel, concat_records
    from specimux_amd.io_utils import SeqRecord
    from specimux_amd.native_io import Lane
    pf, sf, fq = synth_files["c2"]
    both = Both(pf, sf)
    cp = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
    view = U.panel_view(both.opanel)
    NP = len(view.primers)
    assert view.primer_names == cp.primer_names and view.pairs == [tuple(p) for p in cp.pairs] and cp.hits_per_read == 2 * NP
    reads, _ = O.read_sequences(fq)
    bases, offsets, _seqs = concat_records([SeqRecord(s, rid, rid, q) for rid, s, q in reads])
    windows, lens = cp.pack_windows(bases, offsets)
    file_ops = cp.run(windows, lens)[0]
    empty = np.flatnonzero(file_ops["flags"] & _lib.OPF_TRIM_EMPTY)
    others = np.flatnonzero((file_ops["flags"] & _lib.OPF_TRIM_EMPTY) == 0)[:1500]
    assert len(empty) >= 1 and len(others) == 1500
    rows = np.concatenate([np.resize(empty, 4500), others])
    rows = rows[np.random.default_rng(5).permutation(len(rows))]            # interleaved
    small = np.concatenate([others[:97], empty[:1], others[97:99], empty[-1:]])

    def reference_of(batch):
        ops, _extra, _counts, hits, _bdist = cp.run(windows[batch], lens[batch], want_hits="lean")
        return U.rows_reference(NP, view.pdir, view.pairs, True, hits, ops)

    stats = trace_stats.DeviceStats(cp, 1 << 12)
    lane = Lane(cp, 8192)
    counts = np.zeros(cp.counts_len, dtype=np.uint64)
    try:
        lane.attach_stats(stats)
        table = {}
        for batch in (rows, small):
            n = len(batch)
            lane.windows[:n] = windows[batch]
            lane.lens[:n] = lens[batch]
            lane.submit(n)
            ops, _extra = lane.wait(counts)
            flagged = np.flatnonzero(ops["flags"] & _lib.OPF_TRIM_EMPTY).tolist()
            if batch is rows:
                assert 4096 < len(flagged) <= n == 6000
            else:
                assert flagged == [97, 100] and n == 101
            assert sorted(lane.fallback().tolist()) == flagged
            want, listed = reference_of(batch)
            assert listed == flagged
            for key, c in want.items():
                table[key] = table.get(key, 0) + c
            keys, cnts = stats.read()
            assert dict(zip(keys.tolist(), cnts.tolist())) == table
    finally:
        lane.close()
        stats.close()


# ------------------------------------------------------------------ 7: a table that fills up is loud
def test_full_table_is_loud_and_the_tree_stays(lib, tmp_path, synth_files):
    from specimux_amd import cli
    pf, sf, fq = synth_files["c2"]
    table = tmp_path / "t.json"
    res = run_cli([pf, sf, fq, "-F", "-O", tmp_path / "out", "--stats-table", table, "--stats-table-capacity", "8"], check=False)
    assert res.returncode == 1, res.stderr[-2000:]
    assert "--stats-table-capacity" in res.stderr and "filled up" in res.stderr and "--table-capacity)" not in res.stderr
    assert not table.exists() and not any(n.startswith("t.json") for n in os.listdir(tmp_path))
    cli.main(["specimux", pf, sf, fq, "-F", "-O", str(tmp_path / "plain")])
    assert tree_bytes(tmp_path / "out") == tree_bytes(tmp_path / "plain")      # complete, and wrapped up
    assert processed_reads(tmp_path / "out") == 3000


# ------------------------------------------------------------------ 8: two ranks
@pytest.mark.parametrize("mode", ["append", "merge"])
def test_two_rank_table_equals_single_process(lib, tmp_path, synth_files, mode):
    from specimux_amd import cli
    pf, sf, fq = synth_files["c2"]
    exp, _n, _te = oracle_of(pf, sf, fq, "default")
    cli.main(["specimux", pf, sf, fq, "-F", "-O", str(tmp_path / "one"), "--stats-table", str(tmp_path / "one.json")])
    env = dict(os.environ, SMX_DIST_BACKEND="gloo", PYTHONPATH=REPO)
    env.pop("SMX_RANK_MERGE", None)
    if mode == "merge":
        env["SMX_RANK_MERGE"] = "1"
    table = tmp_path / "two.json"
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                          "127.0.0.1", "--master-port", str(29300 + os.getpid() % 200), "-m", "specimux_amd.cli", pf, sf, fq,
                          "-F", "-O", str(tmp_path / "two"), "--stats-table", str(table)], env=env, timeout=600, cwd=REPO,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    one, two = load(tmp_path / "one.json"), load(table)
    assert_tables_equal(two, one, f"two ranks ({mode}) against one process")
    assert_tables_equal(two, exp, f"two ranks ({mode}) against the oracle")
    assert two.host_replayed == one.host_replayed and two.total("sequences") == 3000
    assert sorted(n for n in os.listdir(tmp_path) if n.startswith("two.json")) == ["two.json"]      # no .rank* left
    assert "2 rank tables merged" in (tmp_path / "two" / "log.txt").read_text()


def test_two_rank_full_table_is_loud(lib, tmp_path, synth_files):
    pf, sf, fq = synth_files["c2"]
    table = tmp_path / "two.json"
    table.write_text("left by an earlier run")
    env = dict(os.environ, SMX_DIST_BACKEND="gloo", PYTHONPATH=REPO)
    env.pop("SMX_RANK_MERGE", None)
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                          "127.0.0.1", "--master-port", str(29100 + os.getpid() % 200), "-m", "specimux_amd.cli", pf, sf, fq,
                          "-F", "-O", str(tmp_path / "two"), "--stats-table", str(table), "--stats-table-capacity", "8"],
                         env=env, timeout=600, cwd=REPO, capture_output=True, text=True)
    assert res.returncode != 0
    log = (tmp_path / "two" / "log.txt").read_text()      # rank 0's own message names the flag
    assert "--stats-table-capacity" in log and "filled up" in log and "--table-capacity)" not in log
    assert not any(n.startswith("two.json") for n in os.listdir(tmp_path))      # no table (not the stale one), no rank files
    assert processed_reads(tmp_path / "two") == 3000                            # the tree was wrapped up


# ------------------------------------------------------------------ 9, 10: the watcher's cumulative table
def golden_oracle_table(path, specimens=S):
    both = Both(P, specimens)
    reads, _ = O.read_sequences(path)
    return oracle_table(both.opanel, both.opar, reads)[0]


def test_watcher_table_after_each_file_and_at_the_end(lib, tmp_path, capsys):
    from specimux_amd.trace_stats import StatsTable
    src = tmp_path / "src"
    src.mkdir()
    files = split_fastq(f"{GOLDEN}/sequences.fastq", str(src), GOLDEN_CUTS, ["part1.fastq", "part2.fastq", "part3.fastq"])
    live = tmp_path / "live.json"
    live.write_text("stale")
    w = Watch(tmp_path, ["--stop-after", "3", "-F", "-O", str(tmp_path / "out"), "--stats-table", str(live)])
    assert live.read_text() == "stale"       # replaced at the first success
    so_far = StatsTable()
    for f in files:
        w.drop(f, os.path.basename(f))
        assert w.wait_for(os.path.basename(f)) == "success"
        so_far.merge(golden_oracle_table(f))
        assert_tables_equal(load(live), so_far, f"after {os.path.basename(f)}")
    assert w.join() == 0
    assert load(live).total("sequences") == 40
    capsys.readouterr()
    assert_prints_the_fixtures(live, "golden_default", tmp_path, capsys)
    assert sorted(n for n in os.listdir(tmp_path) if n.startswith("live")) == ["live.json"]


def test_watcher_table_skips_a_failed_file(lib, tmp_path):
    src = tmp_path / "src"
    src.mkdir()
    good = split_fastq(f"{GOLDEN}/sequences.fastq", str(src), [(0, 20), (20, 40)], ["a.fastq", "c.fastq"])
    bad = src / "b.fastq"
    with open(good[0]) as fh:      # valid records first, so that batches of it may have been counted before it fails
        bad.write_text(fh.read() + "@r2\nACGTACGT\nIIIIIIII\n@r3\nACGT\n+\nII\n")
    live = tmp_path / "live.json"
    w = Watch(tmp_path, ["--stop-after", "3", "-F", "-O", str(tmp_path / "out"), "--stats-table", str(live)])
    w.drop(good[0], "a.fastq")
    assert w.wait_for("a.fastq") == "success"
    after_a = live.read_bytes()
    w.drop(str(bad), "b.fastq")
    assert w.wait_for("b.fastq") == "failed"
    assert live.read_bytes() == after_a
    w.drop(good[1], "c.fastq")
    assert w.join() == 0
    assert {os.path.basename(k): v["status"] for k, v in w.state().items()} == {"a.fastq": "success", "b.fastq": "failed",
                                                                                 "c.fastq": "success"}
    exp = golden_oracle_table(good[0]).merge(golden_oracle_table(good[1]))
    assert_tables_equal(load(live), exp, "files 1 + 3")
    assert load(live).total("sequences") == 40


def test_watcher_table_merges_by_name_across_a_reload(lib, tmp_path):
    src = tmp_path / "src"
    src.mkdir()
    files = split_fastq(f"{GOLDEN}/sequences.fastq", str(src), [(0, 20), (20, 40)], ["f1.fastq", "f2.fastq"])
    pf, sf = str(src / "primers.fasta"), str(src / "specimens.txt")
    shutil.copyfile(P, pf)
    shutil.copyfile(S, sf)
    with open(S) as fh:
        original = fh.read()
    # a new first specimen with barcodes of its own: the barcode and specimen numbering of the new panel shifts
    lines = original.rstrip("\n").split("\n")
    edited = "\n".join([lines[0], "TEST_SPECIMEN_000\tITS\tATGCTAGACATCG\tITS1F\tAACGGCCTTGAGG\tITS4"] + lines[1:]) + "\n"
    sf_edit = str(src / "specimens_edit.txt")
    with open(sf_edit, "w") as fh:
        fh.write(edited)
    exp = golden_oracle_table(files[0], sf).merge(golden_oracle_table(files[1], sf_edit))
    live = tmp_path / "live.json"
    w = Watch(tmp_path, ["--stop-after", "2", "-F", "-O", str(tmp_path / "out"), "--stats-table", str(live)], primers=pf, specimens=sf)
    w.drop(files[0], "f1.fastq")
    assert w.wait_for("f1.fastq") == "success"
    with open(sf, "w") as fh:
        fh.write(edited)
    w.drop(files[1], "f2.fastq")
    assert w.join() == 0
    assert_tables_equal(load(live), exp, "two files, two panels")
    assert load(live).total("sequences") == 40
