"""Per-file latency of a live run: one CLI process per file (what the reference's watcher pays, watch.py:131-168) against
the resident watcher (specimux_amd/watch.py).  DESIGN.md section 9 quotes its output.

    python tools/watch_latency.py [--files 20] [--reads 4000] [--stats-table] [--json out.json]

K files of N C2-shaped reads (specimux_amd.synth).  Latency = from the file appearing to its result being usable:
  (a) `python -m specimux_amd.cli P S FILE -F -O out` per file, one after another: the process's wall time (the file is
      there when the process starts; the reference's watcher writes the state entry once the process has exited);
  (b) `python -m specimux_amd.watch P S DIR -F -O out --settle-time 0 --poll-interval 0.05`: a file is renamed into the
      directory once the previous one has its state entry; latency = the entry's timestamp - the rename time.
The watcher's first file is renamed in as soon as the watcher has written its start-up state, which is before it loads
the library and builds the panel: that latency includes HIP start-up and the panel build.  Prints one JSON line."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from datetime import datetime

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from specimux_amd import synth  # noqa: E402


def summary(xs):
    return {"median_s": round(statistics.median(xs), 4), "min_s": round(min(xs), 4), "max_s": round(max(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=20)
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds any one file may take")
    ap.add_argument("--json", default=None)
    ap.add_argument("--stats-table", action="store_true",
                    help="the watcher also keeps its cumulative stats table (--stats-table live.json), rewritten after every file")
    a = ap.parse_args()
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    work = tempfile.mkdtemp(prefix="watch_latency_")
    try:
        pan = synth.panel_c2()
        pf, sf = pan.write(os.path.join(work, "panel"))
        src = os.path.join(work, "src")
        os.makedirs(src)
        files = []
        for i in range(a.files):
            path = os.path.join(src, f"run_{i:03d}.fastq")
            synth.make_reads(pan, a.reads, 9300 + i, windows_only=False).write_fastq(path)
            files.append(path)

        # (a) one CLI process per file
        cli_lat = []
        for f in files:
            t0 = time.perf_counter()
            subprocess.run([sys.executable, "-m", "specimux_amd.cli", pf, sf, f, "-F", "-O", os.path.join(work, "out_cli")],
                           check=True, env=env, cwd=REPO, timeout=a.timeout, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL)
            cli_lat.append(time.perf_counter() - t0)

        # (b) the resident watcher
        wdir, stage = os.path.join(work, "watched"), os.path.join(work, "stage")
        os.makedirs(wdir)
        os.makedirs(stage)
        open(os.path.join(wdir, "before_start.fastq"), "w").close()   # marked ignored: the state file appears at start-up
        state = os.path.join(wdir, ".specimux-watch-state.json")
        t_launch = time.perf_counter()
        watch_cmd = [sys.executable, "-m", "specimux_amd.watch", pf, sf, wdir, "-F", "-O", os.path.join(work, "out_watch"),
                     "--settle-time", "0", "--poll-interval", "0.05", "--stop-after", str(len(files))]
        if a.stats_table:
            watch_cmd += ["--stats-table", os.path.join(work, "live.json")]
        proc = subprocess.Popen(watch_cmd, env=env, cwd=REPO, stdout=subprocess.DEVNULL,
                                stderr=open(os.path.join(work, "watch.log"), "w"))

        def entries():
            try:
                with open(state) as fh:
                    return json.load(fh)["processed_files"]
            except (OSError, ValueError):
                return {}

        def wait(cond, what):
            t0 = time.perf_counter()
            while not cond():
                if proc.poll() is not None and not cond():
                    raise RuntimeError(f"the watcher exited ({proc.returncode}) while waiting for {what}")
                if time.perf_counter() - t0 > a.timeout:
                    raise RuntimeError(f"timed out waiting for {what}")
                time.sleep(0.002)

        try:
            wait(lambda: len(entries()) >= 1, "the start-up state")
            startup_to_state = time.perf_counter() - t_launch
            watch_lat = []
            for f in files:
                tmp = os.path.join(stage, os.path.basename(f))
                shutil.copyfile(f, tmp)
                key = os.path.join(wdir, os.path.basename(f))
                dropped = datetime.now()
                os.rename(tmp, key)
                wait(lambda: key in entries(), os.path.basename(f))
                e = entries()[key]
                if e["status"] != "success":
                    raise RuntimeError(f"{key}: {e['status']}")
                watch_lat.append((datetime.fromisoformat(e["timestamp"]) - dropped).total_seconds())
            proc.wait(timeout=a.timeout)
        finally:
            if proc.poll() is None:
                proc.kill()
                proc.wait()
        if proc.returncode != 0:
            raise RuntimeError(f"the watcher exited with {proc.returncode}")
        same = _tree(os.path.join(work, "out_cli")) == _tree(os.path.join(work, "out_watch"))
        result = {"files": len(files), "reads_per_file": a.reads, "watch_stats_table": bool(a.stats_table),
                  "cli_process_per_file": summary(cli_lat),
                  "watch_first_file": round(watch_lat[0], 4),
                  "watch_later_files": summary(watch_lat[1:]) if len(watch_lat) > 1 else None,
                  "watch_launch_to_startup_state_s": round(startup_to_state, 4),
                  "trees_identical": same,
                  "cli_s": [round(x, 4) for x in cli_lat], "watch_s": [round(x, 4) for x in watch_lat]}
        line = json.dumps(result)
        print(line)
        if a.json:
            with open(a.json, "w") as fh:
                fh.write(line + "\n")
        return 0 if same else 1
    finally:
        shutil.rmtree(work, ignore_errors=True)


def _tree(root):
    out = {}
    for dirpath, _dirs, files in os.walk(root):
        for fn in files:
            if fn != "log.txt":
                with open(os.path.join(dirpath, fn), "rb") as fh:
                    out[os.path.relpath(os.path.join(dirpath, fn), root)] = fh.read()
    return out


if __name__ == "__main__":
    sys.exit(main())
