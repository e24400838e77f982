"""specimux-watch: demultiplex the files of a live sequencing run as they appear (reference: src/specimux/watch.py).

    python -m specimux_amd.watch primers.fasta specimens.txt <minknow dir> -F -O out [-d] [...]

The reference starts one `specimux` process per file (watch.py:131-168).  Here one process keeps what does not change
between files resident: the HIP context, the primer / specimen panel, its match parameters, the compiled panel
(smx_panel) and the three lanes of the streaming pipeline (specimux_amd/pipeline.py).  Each file then goes through
exactly what `python -m specimux_amd.cli primer_file specimen_file FILE <flags>` runs after its start-up
(orchestration.run_native_file for `-F`, orchestration._run_records for `-d` or stdout output), so the output tree is the
one the CLI would leave.  If the primer or specimen file changes (size or mtime), the panel and lanes are rebuilt before
the next file, as the reference's per-file process re-reads both.

Differences from the reference:
  * no `watchdog`: the directory is polled every --poll-interval seconds (this also works on network file systems);
  * a file's settle timer starts when a poll first sees it and keeps running while another file is processed, instead
    of starting only after the previous file is done;
  * an SmxError with SMX_ERR_DEVICE marks the file `failed` and stops the watcher with exit status 1: nothing more is
    launched on a card that may have faulted.
The state file keeps the reference's layout, so tools that read it keep working."""
import argparse
import json
import logging
import os
import signal
import sys
import threading
import time
from datetime import datetime
from pathlib import Path
from typing import Dict, Optional

from . import _lib, cli

STATE_NAME = ".specimux-watch-state.json"
LOG_NAME = "specimux-watch.log"


# ------------------------------------------------------------------ command line (reference: watch.py:307-363)
def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(
        prog="python -m specimux_amd.watch",
        description="Watch directory for new FASTQ files and automatically run specimux.",
        epilog="Example: python -m specimux_amd.watch primers.fasta specimens.txt /path/to/watch -F -O output/ -d")
    parser.add_argument("primer_file", help="Fasta file containing primer information")
    parser.add_argument("specimen_file", help="TSV file containing specimen mapping with barcodes and primers")
    parser.add_argument("watch_dir", help="Directory to watch for new FASTQ files")
    parser.add_argument("--settle-time", type=int, default=30,
                        help="Seconds to wait for file size stability (default: 30)")
    parser.add_argument("--state-file", type=str, default=None,
                        help=f"Path to state file for tracking processed files (default: {STATE_NAME} in watch dir)")
    parser.add_argument("--pattern", type=str, default="*.fastq", help="File pattern to watch (default: *.fastq)")
    parser.add_argument("--daemon", action="store_true", help="Run in daemon mode (log to file instead of stdout)")
    parser.add_argument("--stop-after", type=int, default=None,
                        help="Stop after processing N files (useful for testing)")
    parser.add_argument("--poll-interval", type=float, default=1.0,
                        help="Seconds between two scans of the watch directory (default: 1.0)")
    # the specimux flags, from the CLI's own table: a value the CLI would refuse is refused here, at start-up
    for flags, kwargs in cli._OPTIONS:
        parser.add_argument(*flags, **kwargs)
    return parser


def parse_args(argv):
    """argv[0] is the program name (as for cli.parse_args)."""
    parser = build_parser()
    args = parser.parse_args(argv[1:])
    watch_path = Path(args.watch_dir)
    if not watch_path.exists():
        parser.error(f"Watch directory does not exist: {args.watch_dir}")
    if not watch_path.is_dir():
        parser.error(f"Watch path is not a directory: {args.watch_dir}")
    if args.state_file is None:
        args.state_file = str(watch_path / STATE_NAME)
    if not args.poll_interval > 0:
        parser.error("--poll-interval must be a positive number of seconds")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        parser.error(f"specimux-watch runs in one process on one GPU; it cannot run under a multi-process launch "
                     f"(WORLD_SIZE={world})")
    cli.check_stats_table(parser, args)
    return cli.split_num_seqs(parser, args)


def _specimux_dests():
    return [a.dest for a in cli.build_parser()._actions if a.dest not in ("help", "version")]


def specimux_namespace(args, sequence_file) -> argparse.Namespace:
    """What cli.parse_args gives for `specimux primer_file specimen_file sequence_file <this watch's specimux flags>`."""
    ns = argparse.Namespace()
    for dest in _specimux_dests():
        setattr(ns, dest, str(sequence_file) if dest == "sequence_file" else getattr(args, dest))
    ns.start_seq = args.start_seq
    # --stats-table is the watcher's own: one cumulative table for the live run, never a per-file table that every
    # file's run would overwrite
    for dest, default in _WATCH_OWNED_DEFAULTS.items():
        setattr(ns, dest, default)
    return ns


_WATCH_OWNED_DEFAULTS = {dest: kwargs.get("default") for flags, kwargs in cli._OPTIONS
                         for dest in [flags[-1].lstrip("-").replace("-", "_")] if dest in cli.WATCH_OWNED}


def specimux_flags(args) -> list:
    """This watch's specimux flags as a command line gives them (the reference's build_specimux_args, watch.py:366-405):
    only the flags whose values differ from the defaults."""
    out = []
    for flags, kwargs in cli._OPTIONS:
        dest = flags[-1].lstrip("-").replace("-", "_")
        if dest in cli.WATCH_OWNED:
            continue
        if dest == "num_seqs":
            if args.start_seq != 1:
                out += [flags[0], f"{args.start_seq},{args.num_seqs}"]
            elif args.num_seqs != -1:
                out += [flags[0], str(args.num_seqs)]
            continue
        value = getattr(args, dest)
        if kwargs.get("action") == "store_true":
            if value:
                out.append(flags[0])
        elif value != kwargs.get("default"):
            out += [flags[0], str(value)]
    return out


def setup_logging(daemon: bool, output_dir: Optional[str] = None, debug: bool = False):
    """Console, or with --daemon the file specimux-watch.log (appended) in output_dir or the working directory
    (reference: watch.py:266-304).  There is no fork: --daemon only moves the log."""
    root = logging.getLogger()
    root.handlers.clear()
    fmt = logging.Formatter("%(asctime)s - %(levelname)s - %(message)s")
    if daemon:
        log_dir = Path(output_dir) if output_dir else Path.cwd()
        log_dir.mkdir(parents=True, exist_ok=True)
        log_file = log_dir / LOG_NAME
        handler = logging.FileHandler(log_file, mode="a")
        print(f"Daemon mode: logging to {log_file}")
    else:
        handler = logging.StreamHandler()
    handler.setFormatter(fmt)
    root.addHandler(handler)
    root.setLevel(logging.DEBUG if debug else logging.INFO)


# ------------------------------------------------------------------ state file (reference: watch.py:22-74)
class ProcessedFilesTracker:
    """{"processed_files": {path: {timestamp, size, status}}}, status `success`, `failed` or `ignored`; written after
    every change (to a temporary file first, so that a reader never sees half of it)."""

    def __init__(self, state_file):
        self.state_file = Path(state_file)
        self.processed: Dict[str, dict] = {}
        if self.state_file.exists():
            try:
                with open(self.state_file) as fh:
                    self.processed = json.load(fh).get("processed_files", {})
                logging.info(f"Loaded state: {len(self.processed)} previously processed files")
            except Exception as e:
                logging.warning(f"Could not load state file: {e}")
                self.processed = {}

    def _save_state(self):
        tmp = self.state_file.with_name(self.state_file.name + ".tmp")
        try:
            with open(tmp, "w") as fh:
                json.dump({"processed_files": self.processed}, fh, indent=2)
            os.replace(tmp, self.state_file)
        except Exception as e:
            logging.error(f"Could not save state file: {e}")

    def is_processed(self, filepath: str) -> bool:
        return filepath in self.processed

    def mark_processed(self, filepath: str, status: str, size: int):
        self.processed[filepath] = {"timestamp": datetime.now().isoformat(), "size": size, "status": status}
        self._save_state()

    def get_status(self, filepath: str) -> Optional[str]:
        return self.processed.get(filepath, {}).get("status")


# ------------------------------------------------------------------ what stays resident between files
class _PanelState:
    """Specimens, match parameters, prefilter, compiled panel and (for the streaming path) lanes of one version of the
    primer and specimen files; with --stats-table also the panel's device statistics table and host replay
    (`match_stats`, a trace_stats.RunStats)."""

    def __init__(self, args):
        from . import orchestration
        from .demultiplex import compiled_panel
        self.loaded = orchestration._load(args)
        specimens, parameters, prefilter = self.loaded
        self.specimens = specimens
        self.lanes = []
        self.match_stats = None
        if args.output_to_files and not args.diagnostics:
            from .pipeline import make_lanes
            self.panel = compiled_panel(specimens, parameters, args, prefilter)
            self.lanes = make_lanes(self.panel)
            if getattr(args, "stats_table", None):
                from .trace_stats import RunStats
                try:
                    self.match_stats = RunStats(self.panel, parameters, specimens, args, prefilter is not None,
                                                args.stats_table_capacity)
                except BaseException:
                    self.close()
                    raise
        else:
            # the panel process_sequences asks for on the record path (it finds it in the same cache)
            tracing_or_color = bool(args.diagnostics) or (bool(args.color) and not args.output_to_files)
            self.panel = compiled_panel(specimens, parameters, args, prefilter, want_starts=tracing_or_color)

    def close(self):
        for ln in self.lanes:   # lanes first: they hold a stream slot of their panel
            ln.close()
        self.lanes = []
        if self.match_stats is not None:   # device table and host replay go before their panel
            self.match_stats.close()
            self.match_stats = None
        for panel in self.specimens.__dict__.get("_smx_panels", {}).values():
            panel.close()


def _signature(*paths):
    sig = []
    for p in paths:
        st = os.stat(p)
        sig.append((st.st_size, st.st_mtime_ns))
    return tuple(sig)


class Resident:
    """The panel state of the run, rebuilt when the primer or specimen file has changed (size or st_mtime_ns) since it was
    built: the old panel and lanes are freed first.  `build(args)` returns an object with close()."""

    def __init__(self, args, build=_PanelState):
        self.args = args
        self._build = build
        self.state = None
        self._sig = None
        self.builds = 0

    def current(self):
        sig = _signature(self.args.primer_file, self.args.specimen_file)
        if self.state is not None and sig == self._sig:
            return self.state
        if self.state is not None:
            logging.info("Primer or specimen file changed: reloading the panel")
            self.close()
        self.state = self._build(self.args)
        self._sig = sig
        self.builds += 1
        return self.state

    def close(self):
        if self.state is not None:
            state, self.state = self.state, None
            state.close()


class FileProcessor:
    """One file, as `python -m specimux_amd.cli primer_file specimen_file FILE <flags>` would run it, through the
    resident panel.  With -F, <output_dir>/log.txt is rewritten and holds this file's run log."""

    def __init__(self, args, resident: Resident, live_stats=None):
        self.args, self.resident, self.live_stats = args, resident, live_stats
        self.command = ["specimux", args.primer_file, args.specimen_file, "{}"] + specimux_flags(args)

    def __call__(self, path):
        from . import orchestration
        ns = specimux_namespace(self.args, path)
        handler = None
        if ns.output_to_files:
            os.makedirs(ns.output_dir, exist_ok=True)
            handler = logging.FileHandler(os.path.join(ns.output_dir, "log.txt"), mode="w")
            handler.setFormatter(logging.Formatter("%(asctime)s - %(levelname)s - %(message)s"))
            logging.getLogger().addHandler(handler)
        try:
            logging.info(f"Running: {' '.join(self.command).replace('{}', str(path))}")
            state = self.resident.current()
            if ns.output_to_files and not ns.diagnostics:
                if self.live_stats is None:
                    orchestration.run_native_file(ns, state.specimens, state.panel, state.lanes)
                else:
                    match_stats = state.match_stats
                    match_stats.reset()   # the device table holds one file at a time
                    orchestration.run_native_file(ns, state.specimens, state.panel, state.lanes, match_stats=match_stats)
                    self.live_stats.add_file(match_stats.table)   # reached only when the file succeeded: a failed file adds nothing
            else:
                orchestration._run_records(ns, to_files=ns.output_to_files, loaded=state.loaded)
        finally:
            if handler is not None:
                logging.getLogger().removeHandler(handler)
                handler.close()


class LiveStats:
    """--stats-table FILE: the cumulative stats table of the live run.  It lives on the host as rows of names, so it
    outlives a panel reload (a new panel numbers its primers, barcodes and pools anew; names merge).  Empty at start-up,
    as the state file is; FILE is rewritten (atomically) after every file that succeeded, never after one that failed."""

    def __init__(self, path):
        from .trace_stats import StatsTable
        self.path = path
        self.table = StatsTable()
        self.files = 0

    def add_file(self, table):
        self.table.merge(table)
        self.files += 1
        self.table.save(self.path)
        logging.info(f"Stats table {self.path}: this file {table.total('sequences'):,} reads (host_replayed "
                     f"{table.host_replayed}); {self.table.total('sequences'):,} reads in {len(self.table.counts):,} "
                     f"distinct rows from {self.files} file(s) so far")


# ------------------------------------------------------------------ the poller
class _Pending:
    __slots__ = ("size", "since", "first")

    def __init__(self, size, now):
        self.size, self.since, self.first = size, now, now


class DeviceStop(Exception):
    """A file failed with SMX_ERR_DEVICE: the watcher stops."""


class Watcher:
    """Polls `watch_dir` (no recursion) for files that match `pattern`.  A file is ready once its size has not changed
    for `settle_time` seconds (0: ready when first seen); ready files are processed one at a time in the order polls
    first saw them (ties by name), and each file at most once.  A pending file that disappears is marked `failed`.
    `process(path)` raises on failure; `clock` and `sleep` are injectable (tests)."""

    def __init__(self, watch_dir, pattern, settle_time, poll_interval, tracker, process, stop_after=None,
                 clock=time.monotonic, sleep=time.sleep, exclude=()):
        self.watch_dir, self.pattern = Path(watch_dir), pattern
        self.settle_time, self.poll_interval = settle_time, poll_interval
        self.tracker, self.process, self.stop_after = tracker, process, stop_after
        self.clock, self.sleep = clock, sleep
        self.exclude = set(exclude)
        self.pending: Dict[str, _Pending] = {}
        self.processed_count = 0
        self.interrupted = False

    def scan(self):
        """One poll: new files start settling, a size change restarts a file's timer.  Returns the poll's time."""
        now = self.clock()
        present = set()
        try:
            entries = list(os.scandir(self.watch_dir))
        except OSError as e:
            logging.warning(f"Cannot list {self.watch_dir}: {e}")
            entries = []
        for entry in entries:
            path = self.watch_dir / entry.name
            key = str(path)
            if key in self.exclude or not path.match(self.pattern):
                continue
            try:
                if not entry.is_file():
                    continue
                size = entry.stat().st_size
            except OSError:
                continue   # gone since the listing
            present.add(key)
            if self.tracker.is_processed(key):
                continue
            p = self.pending.get(key)
            if p is None:
                self.pending[key] = _Pending(size, now)
                logging.info(f"New file detected: {entry.name}")
            elif p.size != size:
                logging.debug(f"{entry.name} size changed: {p.size} -> {size} bytes")
                p.size, p.since = size, now
        for key in [k for k in self.pending if k not in present]:
            del self.pending[key]
            logging.warning(f"File {key} disappeared during stability check")
            self.tracker.mark_processed(key, "failed", 0)
        return now

    def next_ready(self, now):
        """The first-seen pending file if it has settled, else None (later files wait for it)."""
        if not self.pending:
            return None
        key = min(self.pending, key=lambda k: (self.pending[k].first, k))
        return key if now - self.pending[key].since >= self.settle_time else None

    def run_one(self, key):
        p = self.pending.pop(key)
        name = Path(key).name
        try:
            size = os.stat(key).st_size
        except OSError:
            logging.warning(f"File {key} disappeared during stability check")
            self.tracker.mark_processed(key, "failed", 0)
            return
        logging.info(f"{name} is stable at {p.size} bytes")
        device_error = None
        try:
            self.process(key)
            status = "success"
            logging.info(f"Successfully processed {name}")
        except Exception as e:
            status = "failed"
            if isinstance(e, _lib.SmxError) and e.code == _lib.ERR_DEVICE:
                device_error = e
            logging.error(f"Specimux failed on {name}: {e}")
            logging.debug("", exc_info=True)
        self.tracker.mark_processed(key, status, size)
        self.processed_count += 1
        logging.info(f"Processed {self.processed_count} file(s) total")
        if device_error is not None:
            raise DeviceStop(str(device_error)) from device_error

    def run(self) -> int:
        """Poll and process until --stop-after, an interrupt (0) or a device error (1)."""
        try:
            while True:
                if self.interrupted:
                    logging.info("Received interrupt, stopping...")
                    return 0
                key = self.next_ready(self.scan())
                if key is None:
                    self.sleep(self.poll_interval)
                    continue
                self.run_one(key)
                if self.stop_after and self.processed_count >= self.stop_after:
                    logging.info(f"Reached stop limit of {self.stop_after} files")
                    logging.info("Stopping after processing requested number of files")
                    return 0
        except DeviceStop as e:
            logging.error(f"Device error: {e}. Stopping; nothing more is launched on this GPU")
            return 1
        except KeyboardInterrupt:   # a second Ctrl-C: the current file was abandoned
            logging.info("Received interrupt, stopping...")
            return 0


# ------------------------------------------------------------------ entry point (reference: watch.py:408-447)
def main(argv=None, process=None, clock=time.monotonic, sleep=time.sleep, on_ready=None) -> int:
    """argv[0] is the program name.  Returns the exit status: 0, or 1 after a start-up error or a device error.
    `process(path)` replaces the resident GPU processor (tests); `on_ready()` is called once the watcher polls."""
    argv = sys.argv if argv is None else argv
    args = parse_args(argv)
    setup_logging(args.daemon, args.output_dir if args.output_to_files else None, args.debug)
    logging.info("Starting specimux-watch")
    logging.info(f"Watching directory: {args.watch_dir}")
    logging.info(f"Pattern: {args.pattern}")
    logging.info(f"Settle time: {args.settle_time}s")
    logging.info(f"Poll interval: {args.poll_interval}s")
    logging.info(f"State file: {args.state_file}")
    logging.info(f"Specimux arguments: {' '.join(specimux_flags(args))}")

    state_file = Path(args.state_file)
    if state_file.exists():
        logging.info("Removing old state file")
        state_file.unlink()
    tracker = ProcessedFilesTracker(state_file)
    existing = list(Path(args.watch_dir).glob(args.pattern))
    if existing:
        logging.info(f"Found {len(existing)} pre-existing file(s) - marking as ignored")
        for path in existing:
            try:
                tracker.mark_processed(str(path), "ignored", path.stat().st_size)
                logging.debug(f"  Ignoring: {path.name}")
            except Exception as e:
                logging.warning(f"Could not stat {path.name}: {e}")

    resident = None
    if process is None:
        # read by libsmx.so: set before it is first loaded.  Without the mapping a shrinking input is a read error, not
        # a SIGBUS that would end the whole watch (smx_io.cpp, smx_reader_open)
        if args.output_to_files and args.threads > 0 and "SMX_IO_THREADS" not in os.environ:
            os.environ["SMX_IO_THREADS"] = str(args.threads)
        os.environ["SMX_IO_NO_MMAP"] = "1"
        if not args.output_to_files and args.threads > 1:
            logging.warning(f"Multithreading only supported for file output. Ignoring --threads {args.threads}")
        resident = Resident(args)
        try:
            t0 = time.perf_counter()
            resident.current()
            logging.info(f"Panel loaded and compiled in {time.perf_counter() - t0:.2f} seconds")
        except Exception as e:
            logging.error(f"Could not load the panel: {e}")
            resident.close()
            return 1
        process = FileProcessor(args, resident, LiveStats(args.stats_table) if args.stats_table else None)

    watcher = Watcher(args.watch_dir, args.pattern, args.settle_time, args.poll_interval, tracker, process,
                      stop_after=args.stop_after, clock=clock, sleep=sleep,
                      exclude=(str(state_file), str(state_file.with_name(state_file.name + ".tmp"))))
    previous_handler = None
    if threading.current_thread() is threading.main_thread():
        def on_sigint(_signum, _frame):
            if watcher.interrupted:   # a second Ctrl-C does not wait for the current file
                raise KeyboardInterrupt
            watcher.interrupted = True
        previous_handler = signal.signal(signal.SIGINT, on_sigint)
    logging.info("Watching for new files (Ctrl+C to stop)...")
    try:
        if on_ready is not None:
            on_ready()
        return watcher.run()
    finally:
        if previous_handler is not None:
            signal.signal(signal.SIGINT, previous_handler)
        if resident is not None:
            resident.close()
        logging.info("Stopped")


if __name__ == "__main__":
    sys.exit(main())
