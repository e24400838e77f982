"""specimux-watch without a GPU: the command line, the state file, settling and ordering, error handling and the
panel-reload rule.  The per-file processor and the clock are fakes, so nothing sleeps for real."""
import json
import logging
import os
import signal

import pytest

from specimux_amd import _lib, cli, watch

P, S = "primers.fasta", "specimens.txt"


class FakeTime:
    """clock() / sleep() for the watcher: sleep advances the clock and then runs the actions scheduled up to then."""

    def __init__(self, limit=1000.0):
        self.t, self.limit, self.actions = 0.0, limit, []

    def at(self, t, fn):
        self.actions.append((t, fn))
        self.actions.sort(key=lambda a: a[0])

    def clock(self):
        return self.t

    def sleep(self, seconds):
        self.t = round(self.t + seconds, 9)
        if self.t > self.limit:
            raise AssertionError(f"the watcher was still polling at t={self.t}")
        while self.actions and self.actions[0][0] <= self.t:
            self.actions.pop(0)[1]()


class FakeProcessor:
    def __init__(self, ft, fail=None):
        self.ft, self.fail, self.calls = ft, fail or {}, []

    def __call__(self, path):
        name = os.path.basename(path)
        self.calls.append((name, self.ft.t))
        if name in self.fail:
            raise self.fail[name]


def write(path, text="@r\nACGT\n+\nIIII\n"):
    with open(path, "a") as fh:
        fh.write(text)


def state_of(watch_dir):
    with open(os.path.join(watch_dir, watch.STATE_NAME)) as fh:
        return json.load(fh)["processed_files"]


def run(tmp_path, flags, ft, proc, ready=None):
    d = tmp_path / "in"
    d.mkdir(exist_ok=True)
    rc = watch.main(["specimux-watch", P, S, str(d)] + flags, process=proc, clock=ft.clock, sleep=ft.sleep,
                    on_ready=ready)
    return rc, str(d)


# ------------------------------------------------------------------ command line
def test_parser_defaults(tmp_path):
    a = watch.parse_args(["specimux-watch", P, S, str(tmp_path)])
    assert (a.primer_file, a.specimen_file, a.watch_dir) == (P, S, str(tmp_path))
    assert a.settle_time == 30 and a.pattern == "*.fastq" and a.daemon is False and a.stop_after is None
    assert a.poll_interval == 1.0
    assert a.state_file == str(tmp_path / ".specimux-watch-state.json")
    assert (a.min_length, a.max_length, a.index_edit_distance, a.primer_edit_distance, a.search_len) == (-1, -1, -1, -1, 80)
    assert (a.output_to_files, a.output_file_prefix, a.output_dir, a.color) == (False, "", ".", False)
    assert (a.trim, a.dereplicate, a.diagnostics, a.debug) == ("barcodes", "best", None, False)
    assert (a.disable_prefilter, a.disable_preorient, a.threads, a.sample_topq) == (False, False, -1, 0)


def test_parser_takes_the_reference_flag_set(tmp_path):
    out, state = str(tmp_path / "out"), str(tmp_path / "st.json")
    a = watch.parse_args(["specimux-watch", P, S, str(tmp_path), "--settle-time", "5", "--state-file", state, "--pattern",
                          "*.fastq*", "--daemon", "--stop-after", "3", "--min-length", "10", "--max-length", "900", "-e", "2",
                          "-E", "3", "-l", "100", "-F", "-P", "p_", "-O", out, "--color", "--trim", "primers", "--dereplicate",
                          "none", "-d", "2", "-D", "--disable-prefilter", "--disable-preorient", "-t", "4", "--sample-topq",
                          "5", "--poll-interval", "0.25"])
    assert (a.settle_time, a.state_file, a.pattern, a.daemon, a.stop_after, a.poll_interval) == (5, state, "*.fastq*", True,
                                                                                                  3, 0.25)
    assert (a.min_length, a.max_length, a.index_edit_distance, a.primer_edit_distance, a.search_len) == (10, 900, 2, 3, 100)
    assert (a.output_to_files, a.output_file_prefix, a.output_dir, a.color, a.trim, a.dereplicate) == (
        True, "p_", out, True, "primers", "none")
    assert (a.diagnostics, a.debug, a.disable_prefilter, a.disable_preorient, a.threads, a.sample_topq) == (
        2, True, True, True, 4, 5)
    assert watch.parse_args(["specimux-watch", P, S, str(tmp_path), "-d"]).diagnostics == 1


@pytest.mark.parametrize("case", ["missing", "file"])
def test_parser_rejects_a_bad_watch_dir(tmp_path, capsys, case):
    target = tmp_path / "nope"
    if case == "file":
        target.write_text("x")
    with pytest.raises(SystemExit) as e:
        watch.parse_args(["specimux-watch", P, S, str(target)])
    assert e.value.code == 2
    want = "Watch directory does not exist: " if case == "missing" else "Watch path is not a directory: "
    assert want + str(target) in capsys.readouterr().err


@pytest.mark.parametrize("bad", [["--trim", "ends"], ["-n", "1,2,3"], ["-d", "4"], ["--poll-interval", "0"],
                                 ["--dereplicate", "all"]])
def test_bad_specimux_flags_fail_at_start_up(tmp_path, bad):
    with pytest.raises(SystemExit) as e:
        watch.main(["specimux-watch", P, S, str(tmp_path)] + bad, process=lambda p: None)
    assert e.value.code == 2
    assert not (tmp_path / watch.STATE_NAME).exists()


def test_multi_process_launch_is_refused(tmp_path, monkeypatch, capsys):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        watch.parse_args(["specimux-watch", P, S, str(tmp_path)])
    assert "WORLD_SIZE=2" in capsys.readouterr().err


FLAG_MATRIX = [
    [],
    ["-F", "-O", "out"],
    ["-F", "-O", "out", "-P", "pfx_", "--trim", "primers", "--dereplicate", "none", "--disable-preorient"],
    ["-F", "-d"],
    ["-d", "3", "--color", "-D"],
    ["-n", "101,500", "-e", "2", "-E", "4", "-l", "120", "--min-length", "100", "--max-length", "2000"],
    ["-n", "25", "--disable-prefilter", "-t", "8", "--sample-topq", "3", "--trim", "tails"],
]


@pytest.mark.parametrize("flags", FLAG_MATRIX)
def test_specimux_namespace_equals_the_cli(tmp_path, flags):
    seq = str(tmp_path / "reads.fastq")
    wargs = watch.parse_args(["specimux-watch", P, S, str(tmp_path)] + flags)
    want = vars(cli.parse_args(["specimux", P, S, seq] + flags))
    assert vars(watch.specimux_namespace(wargs, seq)) == want
    # the command line the watcher logs for a file means the same run
    assert vars(cli.parse_args(["specimux", P, S, seq] + watch.specimux_flags(wargs))) == want


# ------------------------------------------------------------------ start-up and the state file
def test_start_up_clears_state_and_ignores_existing_files(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    (d / watch.STATE_NAME).write_text(json.dumps({"processed_files": {"old.fastq": {"status": "success"}}}))
    write(d / "a.fastq")
    write(d / "b.fastq", "@r\nAC\n+\nII\n")
    write(d / "c.txt")
    ft = FakeTime()
    proc = FakeProcessor(ft)
    ft.at(2, lambda: write(d / "new.fastq"))
    rc, _ = run(tmp_path, ["--settle-time", "0", "--stop-after", "1"], ft, proc)
    assert rc == 0 and proc.calls == [("new.fastq", 2)]
    st = state_of(d)
    assert set(st) == {str(d / "a.fastq"), str(d / "b.fastq"), str(d / "new.fastq")}
    assert {k: v["status"] for k, v in st.items()} == {str(d / "a.fastq"): "ignored", str(d / "b.fastq"): "ignored",
                                                       str(d / "new.fastq"): "success"}
    assert st[str(d / "a.fastq")]["size"] == 15 and st[str(d / "b.fastq")]["size"] == 11
    for entry in st.values():
        assert set(entry) == {"timestamp", "size", "status"}


def test_daemon_appends_to_the_watch_log(tmp_path, monkeypatch):
    out = tmp_path / "out"
    for i in range(2):
        ft = FakeTime()
        ft.at(1, lambda: write(tmp_path / "in" / f"f{i}.fastq"))
        run(tmp_path, ["--settle-time", "0", "--stop-after", "1", "--daemon", "-F", "-O", str(out)], ft, FakeProcessor(ft))
    text = (out / "specimux-watch.log").read_text()
    assert text.count("Starting specimux-watch") == 2 and text.count("Stopped") == 2
    monkeypatch.chdir(tmp_path)
    ft = FakeTime()
    ft.at(1, lambda: write(tmp_path / "in" / "g.fastq"))
    run(tmp_path, ["--settle-time", "0", "--stop-after", "1", "--daemon"], ft, FakeProcessor(ft))
    assert "Watching directory: " in (tmp_path / "specimux-watch.log").read_text()
    logging.getLogger().handlers.clear()


# ------------------------------------------------------------------ settling and ordering
def test_growing_file_waits_until_stable(tmp_path):
    d = tmp_path / "in"
    ft = FakeTime()
    proc = FakeProcessor(ft)
    ft.at(0.5, lambda: write(d / "run.fastq"))
    ft.at(3, lambda: write(d / "run.fastq"))
    ft.at(6, lambda: write(d / "run.fastq"))
    rc, _ = run(tmp_path, ["--settle-time", "5", "--stop-after", "1"], ft, proc)
    assert rc == 0 and proc.calls == [("run.fastq", 11)]
    assert state_of(d)[str(d / "run.fastq")] == {**state_of(d)[str(d / "run.fastq")], "size": 45, "status": "success"}


def test_settle_time_zero_is_ready_when_first_seen(tmp_path):
    d = tmp_path / "in"
    ft = FakeTime()
    proc = FakeProcessor(ft)
    ft.at(2.5, lambda: write(d / "x.fastq"))
    rc, _ = run(tmp_path, ["--settle-time", "0", "--poll-interval", "0.5", "--stop-after", "1"], ft, proc)
    assert proc.calls == [("x.fastq", 2.5)]


def test_vanished_file_is_failed_and_not_counted(tmp_path):
    d = tmp_path / "in"
    ft = FakeTime()
    proc = FakeProcessor(ft)
    ft.at(1, lambda: write(d / "gone.fastq"))
    ft.at(3, lambda: os.remove(d / "gone.fastq"))
    ft.at(4, lambda: write(d / "kept.fastq"))
    rc, _ = run(tmp_path, ["--settle-time", "5", "--stop-after", "1"], ft, proc)
    assert rc == 0 and proc.calls == [("kept.fastq", 9)]
    st = state_of(d)
    assert st[str(d / "gone.fastq")]["status"] == "failed" and st[str(d / "gone.fastq")]["size"] == 0
    assert st[str(d / "kept.fastq")]["status"] == "success"


def test_processing_follows_first_seen_order(tmp_path):
    d = tmp_path / "in"
    ft = FakeTime()
    proc = FakeProcessor(ft)
    ft.at(1, lambda: write(d / "c.fastq"))
    ft.at(2, lambda: (write(d / "b.fastq"), write(d / "a.fastq")))   # one poll sees both: name order
    # y: first seen at 3, growing until 6; z (seen at 4) settles first but waits for it
    ft.at(3, lambda: write(d / "y.fastq"))
    ft.at(4, lambda: (write(d / "y.fastq"), write(d / "z.fastq")))
    ft.at(6, lambda: write(d / "y.fastq"))
    rc, _ = run(tmp_path, ["--settle-time", "2", "--stop-after", "5"], ft, proc)
    assert [c[0] for c in proc.calls] == ["c.fastq", "a.fastq", "b.fastq", "y.fastq", "z.fastq"]
    assert [c[1] for c in proc.calls] == [3, 4, 4, 8, 8]


def test_settle_timers_run_while_a_file_is_processed(tmp_path):
    d = tmp_path / "in"
    ft = FakeTime()

    class Slow(FakeProcessor):
        def __call__(self, path):
            super().__call__(path)
            ft.t += 10   # ten seconds of work on this file

    proc = Slow(ft)
    ft.at(1, lambda: (write(d / "a.fastq"), write(d / "b.fastq")))
    rc, _ = run(tmp_path, ["--settle-time", "5", "--stop-after", "2"], ft, proc)
    assert proc.calls == [("a.fastq", 6), ("b.fastq", 16)]   # b settled during a's ten seconds


def test_a_file_never_runs_twice(tmp_path):
    d = tmp_path / "in"
    ft = FakeTime()
    proc = FakeProcessor(ft)
    ft.at(1, lambda: write(d / "a.fastq"))
    ft.at(3, lambda: write(d / "a.fastq"))   # grows again after it was processed
    ft.at(4, lambda: os.utime(d / "a.fastq"))
    ft.at(6, lambda: write(d / "b.fastq"))
    rc, _ = run(tmp_path, ["--settle-time", "0", "--stop-after", "2"], ft, proc)
    assert [c[0] for c in proc.calls] == ["a.fastq", "b.fastq"]


def test_subdirectories_and_other_names_are_ignored(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    ft = FakeTime()
    proc = FakeProcessor(ft)

    def drop():
        (d / "sub.fastq").mkdir()
        (d / "sub").mkdir()
        write(d / "sub" / "deep.fastq")
        write(d / "notes.txt")
        write(d / "reads.fq")
        write(d / "reads.fastq.gz")

    ft.at(1, drop)
    ft.at(3, lambda: write(d / "last.fastq"))
    rc, _ = run(tmp_path, ["--settle-time", "0", "--stop-after", "1"], ft, proc)
    assert proc.calls == [("last.fastq", 3)]
    assert list(state_of(d)) == [str(d / "last.fastq")]


# ------------------------------------------------------------------ errors and stopping
def test_host_error_fails_the_file_and_the_watch_goes_on(tmp_path):
    d = tmp_path / "in"
    ft = FakeTime()
    proc = FakeProcessor(ft, fail={"a.fastq": ValueError("malformed record"),
                                   "b.fastq": _lib.SmxError(_lib.ERR_ARG, "cannot open")})
    ft.at(1, lambda: [write(d / n) for n in ("a.fastq", "b.fastq", "c.fastq")])
    rc, _ = run(tmp_path, ["--settle-time", "0", "--stop-after", "3"], ft, proc)
    assert rc == 0 and [c[0] for c in proc.calls] == ["a.fastq", "b.fastq", "c.fastq"]
    assert [v["status"] for v in state_of(d).values()] == ["failed", "failed", "success"]


def test_device_error_stops_with_status_1(tmp_path):
    d = tmp_path / "in"
    ft = FakeTime()
    proc = FakeProcessor(ft, fail={"a.fastq": _lib.SmxError(_lib.ERR_DEVICE, "lane batch failed")})
    ft.at(1, lambda: [write(d / n) for n in ("a.fastq", "b.fastq")])
    ft.at(2, lambda: write(d / "c.fastq"))
    rc, _ = run(tmp_path, ["--settle-time", "0"], ft, proc)
    assert rc == 1 and [c[0] for c in proc.calls] == ["a.fastq"]
    st = state_of(d)
    assert list(st) == [str(d / "a.fastq")] and st[str(d / "a.fastq")]["status"] == "failed"


def test_stop_after_counts_runs(tmp_path):
    d = tmp_path / "in"
    ft = FakeTime()
    proc = FakeProcessor(ft, fail={"b.fastq": OSError("permission denied")})
    ft.at(1, lambda: [write(d / f"{n}.fastq") for n in "abcd"])
    rc, _ = run(tmp_path, ["--settle-time", "0", "--stop-after", "3"], ft, proc)
    assert rc == 0 and [c[0] for c in proc.calls] == ["a.fastq", "b.fastq", "c.fastq"]


def test_interrupt_stops_after_the_current_file(tmp_path):
    d = tmp_path / "in"
    out = tmp_path / "out"
    ft = FakeTime()
    seen = []
    guard = signal.signal(signal.SIGINT, lambda *a: seen.append("guard"))   # a watcher that forgot its handler
    try:
        class Interrupted(FakeProcessor):
            def __call__(self, path):
                super().__call__(path)
                os.kill(os.getpid(), signal.SIGINT)
                for _ in range(1000):   # the handler runs between bytecodes of this thread
                    pass
                self.finished = True

        proc = Interrupted(ft)
        ft.at(1, lambda: [write(d / n) for n in ("a.fastq", "b.fastq")])
        rc, _ = run(tmp_path, ["--settle-time", "0", "--daemon", "-F", "-O", str(out)], ft, proc)
    finally:
        restored = signal.signal(signal.SIGINT, guard)
        signal.signal(signal.SIGINT, signal.default_int_handler)
        logging.getLogger().handlers.clear()
    assert restored is not None and not seen
    assert rc == 0 and proc.calls == [("a.fastq", 1)] and proc.finished
    assert state_of(d)[str(d / "a.fastq")]["status"] == "success"
    log = (out / "specimux-watch.log").read_text()
    assert log.index("Successfully processed a.fastq") < log.index("Received interrupt, stopping...") < log.index("Stopped")


# ------------------------------------------------------------------ the resident panel
class FakeState:
    def __init__(self, log, args):
        self.loaded = ("specimens", "parameters", "prefilter")
        self.specimens, self.panel, self.lanes = "specimens", "panel", ["lane"] * 3
        self.log = log
        log.append("build")

    def close(self):
        self.log.append("close")


def test_specimens_change_triggers_one_reload(tmp_path):
    pf, sf = tmp_path / "p.fasta", tmp_path / "s.txt"
    pf.write_text(">p\nACGT\n")
    sf.write_text("SampleID\n")
    args = watch.parse_args(["specimux-watch", str(pf), str(sf), str(tmp_path)])
    log = []
    res = watch.Resident(args, build=lambda a: FakeState(log, a))
    first = res.current()
    assert res.current() is first and log == ["build"]
    st = os.stat(sf)
    os.utime(sf, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    second = res.current()
    assert second is not first and log == ["build", "close", "build"]
    assert res.current() is second and res.current() is second and res.builds == 2
    with open(pf, "a") as fh:   # same mtime, another size
        fh.write(">q\nTTTT\n")
    os.utime(pf, ns=(st.st_atime_ns, os.stat(pf).st_mtime_ns))
    assert res.current() is not second and res.builds == 3
    res.close()
    assert log == ["build", "close", "build", "close", "build", "close"]


def test_file_processor_routes_and_rewrites_log_txt(tmp_path, monkeypatch):
    from specimux_amd import orchestration
    pf, sf = tmp_path / "p.fasta", tmp_path / "s.txt"
    pf.write_text(">p\nACGT\n")
    sf.write_text("SampleID\n")
    out = tmp_path / "out"
    calls = []

    def native(ns, specimens, panel, lanes=None):
        logging.info(f"native {os.path.basename(ns.sequence_file)}")
        calls.append(("native", ns.sequence_file, specimens, panel, len(lanes)))

    def records(ns, to_files, loaded=None):
        calls.append(("records", ns.sequence_file, to_files, loaded))

    monkeypatch.setattr(orchestration, "run_native_file", native)
    monkeypatch.setattr(orchestration, "_run_records", records)
    log = []
    for flags in (["-F", "-O", str(out)], ["-F", "-O", str(out), "-d"], []):
        args = watch.parse_args(["specimux-watch", str(pf), str(sf), str(tmp_path)] + flags)
        watch.setup_logging(False)
        proc = watch.FileProcessor(args, watch.Resident(args, build=lambda a: FakeState(log, a)))
        proc(str(tmp_path / "1.fastq"))
        proc(str(tmp_path / "2.fastq"))
    logging.getLogger().handlers.clear()
    assert calls == [("native", str(tmp_path / "1.fastq"), "specimens", "panel", 3),
                     ("native", str(tmp_path / "2.fastq"), "specimens", "panel", 3),
                     ("records", str(tmp_path / "1.fastq"), True, ("specimens", "parameters", "prefilter")),
                     ("records", str(tmp_path / "2.fastq"), True, ("specimens", "parameters", "prefilter")),
                     ("records", str(tmp_path / "1.fastq"), False, ("specimens", "parameters", "prefilter")),
                     ("records", str(tmp_path / "2.fastq"), False, ("specimens", "parameters", "prefilter"))]
    assert log == ["build"] * 3
    text = (out / "log.txt").read_text()   # the -F -d run's second file: rewritten per file
    assert "2.fastq" in text and "1.fastq" not in text
