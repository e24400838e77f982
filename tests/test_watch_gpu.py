"""specimux-watch on the GPU: the watcher runs in a thread of this process, files are dropped into its directory once it
reports ready, and the tree it leaves is compared byte for byte with `specimux_amd.cli.main` run on the same files one
after another.  Every wait has a wall-clock bound, so a stuck watcher fails the test instead of hanging it."""
import collections
import csv
import ctypes as C
import gzip
import json
import os
import shutil
import threading
import time

import pytest

from conftest import GOLDEN, read_expected_tree
from specimux_amd import _lib, cli, synth, watch

pytestmark = pytest.mark.gpu

P, S = f"{GOLDEN}/primers.fasta", f"{GOLDEN}/specimens.txt"
BOUND = 300   # seconds any one wait may take


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    n = C.c_int(0)
    _lib.check(lib.smx_device_init(0, C.byref(n)))
    return lib


@pytest.fixture
def counted(lib, monkeypatch):
    """Counts smx_panel_create / smx_lane_create through a wrapper on the loaded library."""
    class Counting:
        def __init__(self, real):
            self._real, self.calls = real, collections.Counter()

        def __getattr__(self, name):
            fn = getattr(self._real, name)
            if name not in ("smx_panel_create", "smx_lane_create"):
                return fn

            def wrapped(*a):
                self.calls[name] += 1
                return fn(*a)
            return wrapped

    wrapper = Counting(lib)
    monkeypatch.setattr(_lib, "_lib", wrapper)
    return wrapper


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


def split_fastq(src, dst_dir, cuts, names):
    with open(src) as fh:
        lines = fh.read().split("\n")
    recs = ["\n".join(lines[i:i + 4]) + "\n" for i in range(0, len(lines) - 1, 4)]
    out = []
    for (a, b), name in zip(cuts, names):
        path = os.path.join(dst_dir, name)
        with open(path, "w") as fh:
            fh.write("".join(recs[a:b]))
        out.append(path)
    return out


GOLDEN_CUTS = [(0, 13), (13, 27), (27, 40)]


def tree_bytes(root, skip_trace=False):
    """{relative path: bytes} of every file under root (log.txt excluded), {relative dir: None} of every directory."""
    out = {}
    for dirpath, dirs, files in os.walk(root):
        rel = os.path.relpath(dirpath, root)
        if skip_trace and rel.split(os.sep)[0] == "trace":
            continue
        out[rel + "/"] = None
        for fn in files:
            if fn == "log.txt":
                continue
            with open(os.path.join(dirpath, fn), "rb") as fh:
                out[os.path.join(rel, fn)] = fh.read()
    return out


def cli_runs(files, out, flags, primers=P, specimens=S, gap=0.0):
    for i, f in enumerate(files):
        if i and gap:
            time.sleep(gap)
        cli.main(["specimux", primers, specimens, f, "-F", "-O", str(out)] + flags)


class Watch:
    """watch.main in a thread; drop() renames finished files into the watched directory."""

    def __init__(self, tmp_path, flags, primers=P, specimens=S):
        self.dir = tmp_path / "watched"
        self.stage = tmp_path / "stage"
        self.dir.mkdir()
        self.stage.mkdir()
        self.ready = threading.Event()
        self.rc, self.error = None, None
        argv = ["specimux-watch", primers, specimens, str(self.dir), "--settle-time", "0", "--poll-interval", "0.05"] + flags
        self.thread = threading.Thread(target=self._run, args=(argv,), daemon=True)
        self.thread.start()
        assert self.ready.wait(BOUND), "the watcher did not become ready"
        assert self.error is None, self.error

    def _run(self, argv):
        try:
            self.rc = watch.main(argv, on_ready=self.ready.set)
        except BaseException as e:
            self.error = e
            self.ready.set()

    def drop(self, src, name):
        tmp = self.stage / name
        shutil.copyfile(src, tmp)
        os.rename(tmp, self.dir / name)   # appears complete: --settle-time 0 takes it at the next poll
        return str(self.dir / name)

    def state(self):
        try:
            with open(self.dir / watch.STATE_NAME) as fh:
                return json.load(fh)["processed_files"]
        except (OSError, ValueError):
            return {}

    def wait_for(self, name):
        key, t0 = str(self.dir / name), time.monotonic()
        while key not in self.state():
            assert self.thread.is_alive() or key in self.state(), f"the watcher ended before {name}: {self.error}"
            assert time.monotonic() - t0 < BOUND, f"{name} was not processed within {BOUND} s"
            time.sleep(0.02)
        return self.state()[key]["status"]

    def join(self):
        self.thread.join(BOUND)
        assert not self.thread.is_alive(), "the watcher did not stop"
        assert self.error is None, self.error
        return self.rc


def watch_files(tmp_path, files, flags, names=None, **kw):
    names = names or [os.path.basename(f) for f in files]
    w = Watch(tmp_path, ["--stop-after", str(len(files))] + flags, **kw)
    for f, n in zip(files, names):
        w.drop(f, n)
    assert w.join() == 0
    return w


# ------------------------------------------------------------------ 1, 2: the golden reads in three files
@pytest.mark.parametrize("seqfile", ["sequences.fastq", "sequences_rc.fastq"])
def test_golden_split_equals_sequential_cli(lib, tmp_path, seqfile):
    src = tmp_path / "src"
    src.mkdir()
    files = split_fastq(f"{GOLDEN}/{seqfile}", str(src), GOLDEN_CUTS, ["part1.fastq", "part2.fastq", "part3.fastq"])
    cli_runs(files, tmp_path / "cli", [])
    w = watch_files(tmp_path, files, ["-F", "-O", str(tmp_path / "out")])
    assert set(v["status"] for v in w.state().values()) == {"success"} and len(w.state()) == 3
    got = tree_bytes(tmp_path / "out")
    assert got == tree_bytes(tmp_path / "cli")
    assert "full/ITS2/gITS7-ITS4/primers.fasta" in got and "full/ITS2/primers.txt" in got
    if seqfile == "sequences.fastq":
        assert read_expected_tree(str(tmp_path / "out")) == read_expected_tree(f"{GOLDEN}/expected_output")
    log = (tmp_path / "out" / "log.txt").read_text()   # the last file's run log only
    assert "Processed 13 sequences" in log and "part3.fastq" in log and "part2.fastq" not in log


@pytest.mark.parametrize("flags", [["--trim", "primers", "--dereplicate", "none", "--disable-preorient", "-P", "pfx_"],
                                   ["--sample-topq", "2"]])
def test_golden_split_with_flags(lib, tmp_path, flags):
    src = tmp_path / "src"
    src.mkdir()
    files = split_fastq(f"{GOLDEN}/sequences.fastq", str(src), GOLDEN_CUTS, ["part1.fastq", "part2.fastq", "part3.fastq"])
    cli_runs(files, tmp_path / "cli", flags)
    watch_files(tmp_path, files, ["-F", "-O", str(tmp_path / "out")] + flags)
    got = tree_bytes(tmp_path / "out")
    assert got == tree_bytes(tmp_path / "cli")
    if "--sample-topq" in flags:
        assert any(k.startswith("subsample/") and k.endswith(".fastq") for k in got)
    else:
        assert any(os.path.basename(k).startswith("pfx_") for k in got)


# ------------------------------------------------------------------ 3: one panel, one set of lanes for the whole watch
def test_synthetic_files_share_one_panel_and_lanes(lib, tmp_path, counted):
    pan = synth.panel_c2()
    pf, sf = pan.write(str(tmp_path / "panel"))
    src = tmp_path / "src"
    src.mkdir()
    files = []
    for i in range(5):
        rs = synth.make_reads(pan, 4000, 7100 + i, windows_only=False)
        path = str(src / f"run{i}.fastq")
        rs.write_fastq(path)
        if i == 2:
            with open(path, "rb") as a, gzip.open(path + ".gz", "wb") as b:
                shutil.copyfileobj(a, b)
            os.remove(path)
            path += ".gz"
        files.append(path)
    cli_runs(files, tmp_path / "cli", [], primers=pf, specimens=sf)
    assert counted.calls == {"smx_panel_create": 5, "smx_lane_create": 15}
    counted.calls.clear()
    w = watch_files(tmp_path, files, ["-F", "-O", str(tmp_path / "out"), "--pattern", "*.fastq*"], primers=pf, specimens=sf)
    assert counted.calls == {"smx_panel_create": 1, "smx_lane_create": 3}
    assert [v["status"] for v in w.state().values()] == ["success"] * 5
    got = tree_bytes(tmp_path / "out")
    assert got == tree_bytes(tmp_path / "cli")
    assert sum(len(v) for k, v in got.items() if v and k.startswith("full/ITS/") and k.endswith(".fastq")) > 10000


# ------------------------------------------------------------------ 4: a malformed file fails alone
def test_malformed_file_fails_and_the_watch_goes_on(lib, tmp_path, counted):
    src = tmp_path / "src"
    src.mkdir()
    good = split_fastq(f"{GOLDEN}/sequences.fastq", str(src), [(0, 20), (20, 40)], ["a.fastq", "c.fastq"])
    bad = src / "b.fastq"
    bad.write_text("@r1\nACGTACGT\n+\nIIIIIIII\n@r2\nACGTACGT\nIIIIIIII\n@r3\nACGT\n+\nII\n")
    cli_runs(good, tmp_path / "cli", [])
    counted.calls.clear()
    w = Watch(tmp_path, ["--stop-after", "3", "-F", "-O", str(tmp_path / "out")])
    for path in (good[0], str(bad), good[1]):
        w.drop(path, os.path.basename(path))
    assert w.join() == 0
    assert {os.path.basename(k): v["status"] for k, v in w.state().items()} == {"a.fastq": "success", "b.fastq": "failed",
                                                                                 "c.fastq": "success"}
    assert tree_bytes(tmp_path / "out") == tree_bytes(tmp_path / "cli")
    assert counted.calls == {"smx_panel_create": 1, "smx_lane_create": 3}   # the lanes outlived the failed file


# ------------------------------------------------------------------ 5: an edited specimens.txt takes effect
def test_specimens_edit_between_files_reloads_the_panel(lib, tmp_path, counted):
    src = tmp_path / "src"
    src.mkdir()
    files = split_fastq(f"{GOLDEN}/sequences.fastq", str(src), [(0, 20), (20, 40)], ["f1.fastq", "f2.fastq"])
    pf, sf = str(src / "primers.fasta"), str(src / "specimens.txt")
    shutil.copyfile(P, pf)
    shutil.copyfile(S, sf)
    with open(S) as fh:
        original = fh.read()
    edited = original.rstrip("\n") + "\nTEST_SPECIMEN_004\tITS\tATGCTAGACATCG\tITS1F\tAACGGCCTTGAGG\tITS4\n"
    sf_edit = str(src / "specimens_edit.txt")
    with open(sf_edit, "w") as fh:
        fh.write(edited)
    cli.main(["specimux", pf, sf, files[0], "-F", "-O", str(tmp_path / "cli")])
    cli.main(["specimux", pf, sf_edit, files[1], "-F", "-O", str(tmp_path / "cli")])
    counted.calls.clear()
    w = Watch(tmp_path, ["--stop-after", "2", "-F", "-O", str(tmp_path / "out")], primers=pf, specimens=sf)
    w.drop(files[0], "f1.fastq")
    assert w.wait_for("f1.fastq") == "success"
    with open(sf, "w") as fh:
        fh.write(edited)
    w.drop(files[1], "f2.fastq")
    assert w.join() == 0
    assert counted.calls == {"smx_panel_create": 2, "smx_lane_create": 6}
    assert tree_bytes(tmp_path / "out") == tree_bytes(tmp_path / "cli")


# ------------------------------------------------------------------ 6: -d 1 through the record path
def trace_rows(root):
    files = sorted((root / "trace").glob("*.tsv"))
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows.append([r[1:] for r in csv.reader(fh, delimiter="\t")])
    return rows


def test_trace_files_equal_sequential_cli(lib, tmp_path):
    src = tmp_path / "src"
    src.mkdir()
    files = split_fastq(f"{GOLDEN}/sequences.fastq", str(src), GOLDEN_CUTS, ["part1.fastq", "part2.fastq", "part3.fastq"])
    cli_runs(files, tmp_path / "cli", ["-d", "1"], gap=1.1)
    w = Watch(tmp_path, ["--stop-after", "3", "-F", "-O", str(tmp_path / "out"), "-d", "1"])
    for i, f in enumerate(files):
        if i:
            time.sleep(1.1)   # trace file names have one-second resolution
        w.drop(f, os.path.basename(f))
        assert w.wait_for(os.path.basename(f)) == "success"
    assert w.join() == 0
    want = trace_rows(tmp_path / "cli")
    assert len(want) == 3 and trace_rows(tmp_path / "out") == want
    assert tree_bytes(tmp_path / "out", skip_trace=True) == tree_bytes(tmp_path / "cli", skip_trace=True)
