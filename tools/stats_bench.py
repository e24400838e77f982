#!/usr/bin/env python3
"""Measurements of specimux-stats on the GPU ("Match statistics on the device").

  python tools/stats_bench.py                 device steps on c2 and c3 (765 000 reads) + the end-to-end comparison
  python tools/stats_bench.py --steps-only    the device steps only
  python tools/stats_bench.py --e2e-only      the end-to-end comparison only
  python tools/stats_bench.py --kernel-only c2    accumulate launches and nothing else timed: the target of a counter run,
      rocprofv3 --pmc TCC_ATOMIC_sum --kernel-include-regex stats_kernel -d OUT -- python tools/stats_bench.py --kernel-only c2

Device steps, per 765 000-read batch resident on the device (HIP events, interleaved rounds in one process, median and
minimum): smx_batch_run_device alone, with the lean hit dump, with the dump + smx_stats_accumulate_device; and the
statistics kernel alone with the bytes it must read (24 B per (primer, end) + 32 B per record) over its time as a fraction
of the 8 TB/s HBM peak.
End to end, one FASTQ of 50 000 synthetic c2 reads (and once more with 400 000): `trace_stats --from-run ... --hierarchical pool primer_pair outcome`
against the trace route -- `specimux_amd.cli -F -d 1`, then the host aggregator over its trace.  The two outputs must be
identical; the wall times and their ratio are printed."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
HBM_PEAK = 8.0e12
N_READS = 765_000


def _setup(which):
    import torch
    from parity_utils import Both
    from specimux_amd import _lib, synth, trace_stats
    from specimux_amd.demultiplex import compiled_panel
    pan = {"c2": synth.panel_c2, "c3": synth.panel_c3}[which]()
    d = tempfile.mkdtemp(prefix="stats_bench_")
    pf, sf = pan.write(d)
    both = Both(pf, sf)
    cp = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
    kw = dict(insert_mean=900, insert_sd=250) if which == "c3" else {}
    rs = synth.make_reads(pan, N_READS, 2002, workers=16, **kw)
    dev = torch.device("cuda", 0)
    n = N_READS
    u8 = dict(dtype=torch.uint8, device=dev)
    b = dict(n=n, cp=cp, w=torch.from_numpy(rs.windows(cp.window_stride)).to(dev), l=torch.from_numpy(rs.lens).to(dev),
             ops=torch.zeros(n * 32, **u8), extra=torch.zeros(n * 32, **u8), hits=torch.zeros(n * cp.hits_per_read * 24, **u8),
             small=torch.zeros(2 + n, dtype=torch.int32, device=dev), counts=torch.zeros(cp.counts_len, dtype=torch.int64, device=dev),
             stats=trace_stats.DeviceStats(cp, 1 << 16), lib=_lib.load())
    return b


def _demux(b, hits):
    from specimux_amd import _lib
    _lib.check(b["lib"].smx_batch_run_device(b["cp"].handle, None, b["w"].data_ptr(), b["l"].data_ptr(), b["n"], b["ops"].data_ptr(),
                                            b["extra"].data_ptr(), b["n"], b["small"].data_ptr(), b["counts"].data_ptr(),
                                            b["hits"].data_ptr() if hits else None, None))


def _stats(b):
    b["stats"].accumulate(None, b["hits"].data_ptr(), b["ops"].data_ptr(), b["n"], b["small"].data_ptr() + 8, b["n"],
                          b["small"].data_ptr() + 4)


def _timed(fn, rounds):
    import torch
    out = []
    for _ in range(rounds):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        z.record()
        z.synchronize()
        out.append(a.elapsed_time(z))
    return out


def device_steps(which, rounds=15):
    import torch
    b = _setup(which)
    variants = {"demux": lambda: _demux(b, False), "demux+dump": lambda: _demux(b, True),
                "demux+dump+stats": lambda: (_demux(b, True), _stats(b)), "stats kernel": lambda: _stats(b)}
    for fn in variants.values():   # warm-up: code objects, workspaces
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):        # interleaved rounds
        for k, fn in variants.items():
            times[k] += _timed(fn, 1)
    keys, _c = b["stats"].read()
    need = b["n"] * (b["cp"].hits_per_read * 24 + 32)
    print(f"[{which}] {b['n']:,} reads, {b['cp'].hits_per_read} hit records per read, {len(keys)} distinct rows; {rounds} interleaved rounds")
    for k, v in times.items():
        med, lo = statistics.median(v), min(v)
        line = f"  {k:18s} median {med:8.3f} ms   min {lo:8.3f} ms   {b['n'] / med / 1e6:6.2f} G reads/s"
        if k == "stats kernel":
            line += f"   reads {need / 1e6:.1f} MB -> {need / (med * 1e-3) / 1e12:.2f} TB/s = {100 * need / (med * 1e-3) / HBM_PEAK:.1f}% of the 8 TB/s HBM peak"
        print(line)
    d = statistics.median(times["demux+dump+stats"]) - statistics.median(times["demux+dump"])
    print(f"  stats on top of demux+dump: {d:+.3f} ms per step ({100 * d / statistics.median(times['demux+dump']):+.1f}%)")
    b["stats"].close()


def kernel_only(which, launches=5):
    import torch
    b = _setup(which)
    _demux(b, True)
    torch.cuda.synchronize()
    for _ in range(launches):
        _stats(b)
    torch.cuda.synchronize()
    keys, _c = b["stats"].read()
    print(f"[{which}] {launches} statistics launches over {b['n']:,} reads, {len(keys)} distinct rows")


def end_to_end(n=50_000):
    from specimux_amd import synth
    d = tempfile.mkdtemp(prefix="stats_e2e_")
    pan = synth.panel_c2()
    pf, sf = pan.write(d)
    fq = os.path.join(d, "reads.fastq")
    synth.make_reads(pan, n, 50_050, windows_only=False).write_fastq(fq)
    env = dict(os.environ, PYTHONPATH=REPO)
    dims = ["--hierarchical", "pool", "primer_pair", "outcome"]

    def run(argv):
        print(f"  running {' '.join(argv[:2])} ...", flush=True)
        t = time.perf_counter()
        res = subprocess.run([sys.executable, "-m"] + argv, cwd=REPO, env=env, capture_output=True, text=True, timeout=3000)
        if res.returncode != 0:
            raise SystemExit(f"{argv[:2]} failed:\n{res.stderr[-2000:]}")
        for line in res.stderr.splitlines():
            if "Counted" in line:
                print("    " + line)
        return res.stdout, time.perf_counter() - t
    run(["specimux_amd.trace_stats", "--from-run", pf, sf, fq, "-n", "1000"] + dims)      # warm the file cache and the machine
    direct, t_direct = run(["specimux_amd.trace_stats", "--from-run", pf, sf, fq] + dims)
    out = os.path.join(d, "out")
    _o, t_cli = run(["specimux_amd.cli", pf, sf, fq, "-F", "-O", out, "-d", "1"])
    via_trace, t_agg = run(["specimux_amd.trace_stats", os.path.join(out, "trace")] + dims)
    size = sum(os.path.getsize(os.path.join(out, "trace", f)) for f in os.listdir(os.path.join(out, "trace")))
    print(f"[end to end] {n:,} c2 reads, --hierarchical pool primer_pair outcome (process wall times, start-up included)")
    print(f"  --from-run                    {t_direct:8.2f} s")
    print(f"  cli -F -d 1 + aggregator      {t_cli + t_agg:8.2f} s   ({t_cli:.2f} s run, {t_agg:.2f} s aggregation, trace {size / 1e6:.1f} MB)")
    print(f"  ratio                         {(t_cli + t_agg) / t_direct:8.1f} x")
    print(f"  outputs identical             {direct == via_trace}")
    if direct != via_trace:
        raise SystemExit("the two routes disagree")


def grid_sweep(which, rounds=15):
    """The statistics kernel alone at 1, 2, 4, 8 workgroups per CU (SMX_STATS_BLOCKS_PER_CU), interleaved."""
    import torch
    b = _setup(which)
    _demux(b, True)
    torch.cuda.synchronize()
    times = {g: [] for g in (1, 2, 4, 8)}
    for r in range(rounds + 1):
        for g in times:
            os.environ["SMX_STATS_BLOCKS_PER_CU"] = str(g)
            t = _timed(lambda: _stats(b), 1)
            if r:
                times[g] += t
    os.environ.pop("SMX_STATS_BLOCKS_PER_CU")
    print(f"[{which}] statistics kernel by workgroups per CU: " +
          ", ".join(f"{g}: {statistics.median(v):.3f} ms (min {min(v):.3f})" for g, v in times.items()))
    b["stats"].close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--e2e-only", action="store_true")
    ap.add_argument("--kernel-only", choices=["c2", "c3"])
    ap.add_argument("--grid-sweep", action="store_true", help="the statistics kernel at 1, 2, 4, 8 workgroups per CU")
    args = ap.parse_args()
    from specimux_amd import _lib
    _lib.check(_lib.load().smx_device_init(0, C.byref(C.c_int(0))))
    if args.kernel_only:
        return kernel_only(args.kernel_only)
    if args.grid_sweep:
        return [grid_sweep(which) for which in ("c2", "c3")]
    if not args.e2e_only:
        for which in ("c2", "c3"):
            device_steps(which)
    if not args.steps_only:
        end_to_end()
        end_to_end(400_000)    # the same comparison where process start-up no longer dominates --from-run


if __name__ == "__main__":
    main()
