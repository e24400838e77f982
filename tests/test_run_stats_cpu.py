"""`--stats-table` without a GPU: the command lines, StatsTable.merge against the reference's committed traces, the atomic
save, the rank-table merge of a sharded run and the watcher's cumulative table (fake panel state and run, as
tests/test_watch_cpu.py does)."""
import csv
import glob
import json
import os

import pytest

from specimux_amd import cli, trace_stats, watch
from stats_utils import CASES, unpack_trace

P, S = "primers.fasta", "specimens.txt"


# ------------------------------------------------------------------ command lines
def test_cli_parser_takes_the_flag_with_F():
    a = cli.parse_args(["specimux", P, S, "reads.fastq", "-F", "-O", "out", "--stats-table", "t.json"])
    assert a.stats_table == "t.json" and a.stats_table_capacity == trace_stats.DEFAULT_TABLE_CAPACITY
    a = cli.parse_args(["specimux", P, S, "reads.fastq", "-F", "--stats-table", "t.json", "--stats-table-capacity", "4096"])
    assert a.stats_table_capacity == 4096
    assert cli.parse_args(["specimux", P, S, "reads.fastq", "-F"]).stats_table is None


@pytest.mark.parametrize("flags", [["--stats-table", "t.json"], ["-F", "-d", "--stats-table", "t.json"],
                                   ["-F", "-d", "2", "--stats-table", "t.json"], ["--stats-table", "t.json", "-d"],
                                   ["-F", "--stats-table", "t.json", "--stats-table-capacity", "0"]])
def test_cli_parser_errors(flags, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["specimux", P, S, "reads.fastq"] + flags)
    assert e.value.code == 2 and "--stats-table" in capsys.readouterr().err


def test_watch_parser_takes_the_flag_and_keeps_it_to_itself(tmp_path, capsys):
    table = str(tmp_path / "live.json")
    a = watch.parse_args(["specimux-watch", P, S, str(tmp_path), "-F", "-O", "out", "--stats-table", table,
                          "--stats-table-capacity", "1024"])
    assert a.stats_table == table and a.stats_table_capacity == 1024
    # a file's run never gets the flag: it would overwrite the cumulative table with its own
    ns = watch.specimux_namespace(a, "x.fastq")
    assert ns.stats_table is None and ns.stats_table_capacity == trace_stats.DEFAULT_TABLE_CAPACITY
    assert vars(ns) == vars(cli.parse_args(["specimux", P, S, "x.fastq", "-F", "-O", "out"]))
    assert not any("stats-table" in f for f in watch.specimux_flags(a))
    for bad in (["--stats-table", table], ["-F", "-d", "--stats-table", table]):
        with pytest.raises(SystemExit) as e:
            watch.parse_args(["specimux-watch", P, S, str(tmp_path)] + bad)
        assert e.value.code == 2 and "--stats-table" in capsys.readouterr().err


def test_stats_tool_parser_is_unchanged(capsys):
    parser = trace_stats.build_parser()
    a = parser.parse_args(["--from-run", P, S, "reads.fastq", "--hierarchical", "pool", "--table-capacity", "64"])
    assert a.table_capacity == 64 and not hasattr(a, "stats_table") and not hasattr(a, "stats_table_capacity")
    with pytest.raises(SystemExit):
        parser.parse_args(["--from-run", P, S, "reads.fastq", "--hierarchical", "pool", "--stats-table", "t.json"])
    capsys.readouterr()
    for flag in ("--min-length", "--max-length", "--num-seqs", "--index-edit-distance", "--primer-edit-distance", "--search-len",
                 "--trim", "--dereplicate", "--disable-prefilter", "--disable-preorient", "--table", "--save-table"):
        assert flag in parser.format_help()
    for flag in ("--output-to-files", "--diagnostics", "--sample-topq", "--stats-table"):
        assert flag not in parser.format_help()


# ------------------------------------------------------------------ StatsTable.merge
def _split_trace(trace_dir, tmp_path, tag):
    """The trace's events in two trace directories, split by sequence id (alternating in order of first appearance)."""
    (src,) = glob.glob(os.path.join(trace_dir, "specimux_trace_*.tsv"))
    with open(src, newline="") as fh:
        header, *rows = list(csv.reader(fh, delimiter="\t"))
    side = {}
    for r in rows:
        side.setdefault(r[3], len(side) % 2)
    dirs = []
    for k in (0, 1):
        d = tmp_path / f"{tag}_half{k}"
        d.mkdir()
        with open(d / "specimux_trace_half_main.tsv", "w", newline="") as fh:
            w = csv.writer(fh, delimiter="\t", lineterminator="\n")
            w.writerow(header)
            w.writerows(r for r in rows if side[r[3]] == k)
        dirs.append(os.fspath(d))
    assert len(side) >= 2
    return dirs


@pytest.mark.parametrize("case", CASES)
def test_merge_of_two_halves_equals_the_whole(case, tmp_path):
    trace = unpack_trace(case, tmp_path)
    whole = trace_stats.table_from_trace_dir(trace)
    a, b = (trace_stats.table_from_trace_dir(d) for d in _split_trace(trace, tmp_path, case))
    assert a.total() and b.total() and a != whole and b != whole
    a.host_replayed, b.host_replayed = 3, 4
    merged = trace_stats.StatsTable().merge(a).merge(b)
    assert merged == whole and merged.counts == whole.counts
    assert merged.total("sequences") == whole.total("sequences") == a.total("sequences") + b.total("sequences")
    assert merged.host_replayed == 7 and (a.host_replayed, b.host_replayed) == (3, 4)
    assert a.merge(b) is a and a == whole                     # in place, returns self
    assert trace_stats.StatsTable.from_json(json.loads(json.dumps(merged.to_json()))) == whole


# ------------------------------------------------------------------ StatsTable.save is atomic
def _table(*rows):
    t = trace_stats.StatsTable()
    for name, first, n in rows:
        t.add((name,) + trace_stats._DEFAULT_ROW[1:], first, n)
    return t


def test_save_is_atomic(tmp_path, monkeypatch):
    path = tmp_path / "t.json"
    old = _table(("forward", True, 5))
    old.save(path)
    before = path.read_bytes()
    assert os.listdir(tmp_path) == ["t.json"]
    real_dump = json.dump

    def half_way(doc, fh, **kw):
        fh.write(json.dumps(doc)[:25])
        fh.flush()
        raise OSError("disk full")

    monkeypatch.setattr(trace_stats.json, "dump", half_way)
    with pytest.raises(OSError, match="disk full"):
        _table(("reverse", True, 9)).save(path)
    assert path.read_bytes() == before and os.listdir(tmp_path) == ["t.json"]    # previous table, no temporary file
    monkeypatch.setattr(trace_stats.json, "dump", real_dump)
    new = _table(("reverse", True, 9))
    new.save(os.fspath(path))
    assert trace_stats.StatsTable.load(path) == new and os.listdir(tmp_path) == ["t.json"]


# ------------------------------------------------------------------ rank tables of a sharded run
def test_rank_tables_merge_into_one(tmp_path):
    path = os.fspath(tmp_path / "run.json")
    a, b = _table(("forward", True, 5), ("unknown", False, 2)), _table(("forward", True, 1), ("reverse", True, 4))
    a.host_replayed, b.host_replayed = 1, 2
    a.save(trace_stats.rank_table_path(path, 0))
    b.save(trace_stats.rank_table_path(path, 1))
    assert sorted(os.listdir(tmp_path)) == ["run.json.rank0", "run.json.rank1"]
    merged = trace_stats.merge_rank_tables(path, 2)
    assert os.listdir(tmp_path) == ["run.json"]
    want = _table(("forward", True, 6), ("unknown", False, 2), ("reverse", True, 4))
    assert merged == want and trace_stats.StatsTable.load(path) == want
    assert trace_stats.StatsTable.load(path).host_replayed == 3


def test_missing_rank_table_is_an_error(tmp_path):
    path = os.fspath(tmp_path / "run.json")
    _table(("forward", True, 5)).save(trace_stats.rank_table_path(path, 0))
    _table(("forward", True, 5)).save(trace_stats.rank_table_path(path, 2))
    with pytest.raises(FileNotFoundError, match="rank 1"):
        trace_stats.merge_rank_tables(path, 3)
    assert os.listdir(tmp_path) == []      # no table, and nothing of the failed run left behind


# ------------------------------------------------------------------ the watcher's cumulative table
class FakeRunStats:
    def __init__(self, log):
        self.table, self.log = trace_stats.StatsTable(), log

    def reset(self):
        self.table = trace_stats.StatsTable()
        self.log.append("reset")

    def close(self):
        self.log.append("stats closed")


class FakeState:
    def __init__(self, log, args):
        self.loaded = ("specimens", "parameters", "prefilter")
        self.specimens, self.panel, self.lanes = "specimens", f"panel{log.count('build')}", ["lane"] * 3
        self.match_stats = FakeRunStats(log)
        self.log = log
        log.append("build")

    def close(self):
        self.log.append("close")


def test_watcher_keeps_one_cumulative_table(tmp_path, monkeypatch):
    from specimux_amd import orchestration
    pf, sf = tmp_path / "p.fasta", tmp_path / "s.txt"
    pf.write_text(">p\nACGT\n")
    sf.write_text("SampleID\n")
    live = tmp_path / "live.json"
    live.write_text("left over from an earlier watch")
    # what each file's run counts; rows are names: specimen B appears with the reloaded panel
    per_file = {"1.fastq": _table(("forward", True, 10), ("unknown", True, 1)),
                "2.fastq": OSError("truncated record"),
                "3.fastq": _table(("forward", True, 7)),
                "4.fastq": _table(("forward", True, 2), ("reverse", True, 3))}
    per_file["1.fastq"].host_replayed = 1
    per_file["4.fastq"].host_replayed = 2
    panels = []

    def native(ns, specimens, panel, lanes=None, match_stats=None):
        assert ns.stats_table is None                   # the file's own run does not write a table
        assert match_stats.table.total() == 0           # reset before every file
        panels.append(panel)
        what = per_file[os.path.basename(ns.sequence_file)]
        match_stats.table.add(("half", ) + trace_stats._DEFAULT_ROW[1:], True, 99)   # counted before the failure
        if isinstance(what, Exception):
            raise what
        match_stats.table = what

    monkeypatch.setattr(orchestration, "run_native_file", native)
    args = watch.parse_args(["specimux-watch", str(pf), str(sf), str(tmp_path), "-F", "-O", str(tmp_path / "out"),
                             "--stats-table", str(live)])
    log = []
    watch.setup_logging(False)
    resident = watch.Resident(args, build=lambda a: FakeState(log, a))
    stats = watch.LiveStats(args.stats_table)
    proc = watch.FileProcessor(args, resident, stats)
    assert live.read_text() == "left over from an earlier watch"      # replaced at the first success, not before

    proc(str(tmp_path / "1.fastq"))
    assert trace_stats.StatsTable.load(live) == per_file["1.fastq"]
    after_first = live.read_bytes()
    with pytest.raises(OSError):
        proc(str(tmp_path / "2.fastq"))
    assert live.read_bytes() == after_first                            # a failed file adds nothing
    proc(str(tmp_path / "3.fastq"))
    assert trace_stats.StatsTable.load(live) == _table(("forward", True, 17), ("unknown", True, 1))
    st = os.stat(sf)
    os.utime(sf, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))   # an edited specimens.txt: the panel is rebuilt
    proc(str(tmp_path / "4.fastq"))
    import logging
    logging.getLogger().handlers.clear()
    assert panels == ["panel0", "panel0", "panel0", "panel1"] and log.count("build") == 2
    final = trace_stats.StatsTable.load(live)
    assert final == _table(("forward", True, 19), ("unknown", True, 1), ("reverse", True, 3)) and final.host_replayed == 3
    assert final == stats.table and stats.files == 3
    assert sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("live")) == ["live.json"]


def test_watcher_without_the_flag_calls_the_run_as_before(tmp_path, monkeypatch):
    from specimux_amd import orchestration
    pf, sf = tmp_path / "p.fasta", tmp_path / "s.txt"
    pf.write_text(">p\nACGT\n")
    sf.write_text("SampleID\n")
    calls = []
    monkeypatch.setattr(orchestration, "run_native_file", lambda *a, **k: calls.append((len(a), k)))
    args = watch.parse_args(["specimux-watch", str(pf), str(sf), str(tmp_path), "-F", "-O", str(tmp_path / "out")])
    watch.setup_logging(False)
    log = []
    watch.FileProcessor(args, watch.Resident(args, build=lambda a: FakeState(log, a)))(str(tmp_path / "1.fastq"))
    import logging
    logging.getLogger().handlers.clear()
    assert calls == [(4, {})] and "reset" not in log
