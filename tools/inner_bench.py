#!/usr/bin/env python3
"""Measurements of the inner scan (smx_inner_scan, specimux-chimera).

  python tools/inner_bench.py                  kernel times on both panels + the end-to-end comparison
  python tools/inner_bench.py --kernel-only    the kernel times only
  python tools/inner_bench.py --e2e-only       the end-to-end comparison only
  python tools/inner_bench.py --reads N        fewer reads (default 765 000)

Kernel: synthetic reads of specimux_amd/synth.py at the bench shape (765 000 reads of about 650 nt; the end windows come
from the generator, the bases between them are random ACGT), the 2-primer panel c2 (4 patterns) and the 8-primer panel
c3 (16 patterns), thresholds min(demux threshold, 3), margin 80, H = 4.  The device time of the kernels of one
smx_inner_scan call (HIP events, summed over the call's chunks; median and minimum of the repeats) next to the two
algorithmic minima: the read bases once from HBM at 8 TB/s, and word-steps x instructions per step over the VALU issue
peak (1024 SIMDs x 2.4 GHz / 2 cycles per wave instruction), word-steps = (columns a lane walks, warm-up included) x
pattern slots / 64 lanes.
End to end, one FASTQ of the same reads: `specimux_amd.chimera --report` (and once more with --clean / --flagged) next to
`specimux_amd.cli -F` on the same file, each in a fresh process, wall time."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_PEAK = 8.0e12
VALU_PEAK = 1024 * 2.4e9 / 2     # wave instructions per second
# VALU instructions of one column step of one pattern in the 32-bit kernel's hot loop (the step itself, the score update
# and the threshold compare), read off the gfx950 ISA
INSTR_PER_STEP = 24


def piece_len(lead):
    """inner_piece_len of specimux_amd/csrc/smx_inner_core.h."""
    pl = 64
    while pl < 4 * lead and pl < 512:
        pl *= 2
    return pl


def full_reads(rs, seed):
    """bases (uint8) and offsets (uint64) of the read set: head window + random ACGT + tail window."""
    lens = rs.lens.astype(np.int64)
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(off[-1]), dtype=np.uint8)]
    S = rs.head.shape[1]
    o = off[:-1].astype(np.int64)
    for lo in range(0, len(lens), 65536):
        hi = min(len(lens), lo + 65536)
        sp = np.minimum(lens[lo:hi], S)
        j = np.arange(S)[None, :]
        ok = j < sp[:, None]
        bases[(o[lo:hi, None] + j)[ok]] = rs.head[lo:hi][ok]
        bases[(o[lo:hi, None] + (lens[lo:hi] - sp)[:, None] + j)[ok]] = rs.tail[lo:hi][ok]
    return bases, off


def load(which, n_reads, directory):
    from specimux_amd import chimera, synth
    pan = {"c2": synth.panel_c2, "c3": synth.panel_c3}[which]()
    pf, sf = pan.write(os.path.join(directory, which))
    args = chimera.parse_args([pf, sf, "unused.fastq"])
    info = chimera.panel_patterns(*chimera.load_panel(args), args.inner_edit_distance)
    rs = synth.make_reads(pan, n_reads, 2002, workers=16)
    return pf, sf, info, rs


def kernel_bench(which, n_reads, repeats, directory):
    from specimux_amd import chimera
    _pf, _sf, info, rs = load(which, n_reads, directory)
    bases, off = full_reads(rs, 7)
    ks = [p.k for p in info]
    margin, H = 80, 4
    lead = max(len(p.seq) + p.k for p in info)
    PL = piece_len(lead)
    inner = np.maximum(rs.lens.astype(np.int64) - 2 * margin, 0)
    pieces = (inner + PL - 1) // PL
    slots = len(info) if len(info) <= 4 else 8 * ((len(info) + 7) // 8)
    columns = int(inner.sum() + lead * pieces.sum())       # an upper bound: a first piece walks min(lead, margin) extra
    word_steps = columns * slots
    t_hbm = len(bases) / HBM_PEAK
    t_valu = word_steps / 64 * INSTR_PER_STEP / VALU_PEAK
    ms, wall = [], []
    for _ in range(repeats + 1):
        got = []
        t0 = time.perf_counter()
        nhit, _, _ = chimera.scan(bases, off, info, ks, margin, H, kernel_ms=got)
        wall.append(time.perf_counter() - t0)
        ms.append(got[0])
    ms, wall = ms[1:], wall[1:]
    print(f"[{which}] {n_reads} reads, {len(bases) / 1e6:.0f} MB, mean {len(bases) / n_reads:.0f} nt; {len(info)} patterns "
          f"({slots} slots), lead {lead}, piece {PL}, {int(pieces.sum())} units; reads with a hit {int(nhit.any(axis=1).sum())}")
    print(f"[{which}] kernels (HIP events, whole call): median {statistics.median(ms):.2f} ms, min {min(ms):.2f} ms over {len(ms)} calls; "
          f"call wall (pageable copies in and out included) median {statistics.median(wall) * 1e3:.0f} ms")
    print(f"[{which}] minima: bases once from HBM {t_hbm * 1e3:.3f} ms; {word_steps / 1e9:.2f} G word-steps x {INSTR_PER_STEP} "
          f"instructions / 64 lanes over the VALU issue peak {t_valu * 1e3:.2f} ms -> bound by "
          f"{'VALU issue' if t_valu > t_hbm else 'HBM'}; kernel time = {min(ms) / (max(t_valu, t_hbm) * 1e3):.2f} x that minimum")


def e2e_bench(n_reads, directory):
    pf, sf, _info, rs = load("c2", n_reads, directory)
    bases, off = full_reads(rs, 7)
    fq = os.path.join(directory, "reads.fastq")
    raw = bases.tobytes()
    qual = (np.random.default_rng(3).integers(3, 41, int(rs.lens.max()) + 4096) + 33).astype(np.uint8).tobytes()
    o = off.tolist()
    with open(fq, "wb") as fh:
        for lo in range(0, n_reads, 8192):
            fh.write(b"".join(b"@read%07d synthetic\n%b\n+\n%b\n" % (i, raw[o[i]:o[i + 1]], qual[i & 4095:(i & 4095) + o[i + 1] - o[i]])
                              for i in range(lo, min(n_reads, lo + 8192))))
    size = os.path.getsize(fq)
    env = dict(os.environ, PYTHONPATH=REPO)

    def timed(cmd):
        t0 = time.perf_counter()
        done = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, errors="replace", timeout=600)
        if done.returncode != 0:
            raise SystemExit(f"{' '.join(cmd)}\nexit status {done.returncode}; the end of its output:\n{done.stdout[-3000:]}")
        return time.perf_counter() - t0

    out = os.path.join(directory, "out")
    t_cli = timed([sys.executable, "-m", "specimux_amd.cli", pf, sf, fq, "-F", "-O", out])
    rep = os.path.join(directory, "report.tsv")
    t_scan = timed([sys.executable, "-m", "specimux_amd.chimera", pf, sf, fq, "--report", rep])
    t_split = timed([sys.executable, "-m", "specimux_amd.chimera", pf, sf, fq, "--report", rep, "--clean",
                     os.path.join(directory, "clean.fastq"), "--flagged", os.path.join(directory, "flagged.fastq")])
    with open(rep) as fh:
        rows = sum(1 for _ in fh) - 1
    print(f"[e2e] {n_reads} reads, FASTQ of {size / 1e6:.0f} MB, each command a fresh process (wall):")
    print(f"[e2e] specimux_amd.cli -F                       {t_cli:7.2f} s")
    print(f"[e2e] specimux_amd.chimera --report             {t_scan:7.2f} s  ({t_scan / t_cli:.2f} x the -F run; {rows} report rows)")
    print(f"[e2e] specimux_amd.chimera --clean --flagged    {t_split:7.2f} s  (the split is written by libsmx batch by batch: "
          f"{n_reads / max(t_split - t_scan, 1e-9) / 1e3:.0f} k records/s, {size / max(t_split - t_scan, 1e-9) / 1e6:.0f} MB/s on top of the scan)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=765_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--e2e-only", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="inner_bench_") as d:
        if not args.e2e_only:
            for which in ("c2", "c3"):
                kernel_bench(which, args.reads, args.repeats, d)
        if not args.kernel_only:
            e2e_bench(args.reads, d)


if __name__ == "__main__":
    main()
