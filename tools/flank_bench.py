#!/usr/bin/env python3
"""Measurements of the barcode survey's two kernels (smx_flank.hip, specimux-barcodes).

  python tools/flank_bench.py                  765 000 synthetic c2 reads (32 x 24 barcodes, ITS1F / ITS4)
  python tools/flank_bench.py --reads N        fewer reads
  python tools/flank_bench.py --withhold 4     the sheet lacks the last 4 forward and reverse barcodes (novel candidates)

The reads go through the demux kernel once, in one batch, with the hit dump; windows, lengths and hits stay on the device.
flank_count_kernel: HIP-event time of smx_flank_accumulate_device over that batch into an empty table (median and minimum
of the repeats, the table cleared between them), next to what the kernel must read from HBM: every hit record (24 bytes
per (read, primer, end)), the read lengths (4 bytes per read) and, per counted hit, the 128-byte lines its flank of at
most 26 bytes touches (one, sometimes two), at 8 TB/s.  The table traffic is on top of that floor.
flank_assign_kernel: the kernel_ms of one smx_flank_assign call over the distinct keys and the candidates the tool would
pass (listed barcodes, then unlisted peaks of at least --min-count copies), next to the VALU minimum: (key, candidate) pairs
x flank columns x instructions per column over the issue peak (1024 SIMDs x 2.4 GHz / 2 cycles per wave instruction)."""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_PEAK = 8.0e12
VALU_PEAK = 1024 * 2.4e9 / 2     # wave instructions per second
INSTR_PER_COLUMN = 20            # VALU instructions of one flank_shw column (match-word select, step, score, minimum)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=765_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--withhold", type=int, default=0)
    ap.add_argument("--min-count", type=int, default=10)
    args = ap.parse_args()
    import torch
    from specimux_amd import _lib, barcodes, synth, trace_stats
    lib = _lib.load()
    full = synth.panel_c2()
    w = args.withhold
    sheet = synth.Panel(full.pools, full.fwd[:len(full.fwd) - w], full.rev[:len(full.rev) - w])
    with tempfile.TemporaryDirectory(prefix="flank_bench_") as d:
        pf, sf = sheet.write(d)
        # specimux's default flags (an empty namespace overrides none); the two files are read here and not again, and no
        # sequence file is opened: the reads below come from the generator
        _ns, specs, _par, _pre, panel = trace_stats.load_run_panel(pf, sf, None, argparse.Namespace())
    n = args.reads
    rs = synth.make_reads(full, n, 2002, workers=16)
    windows = torch.from_numpy(rs.windows(panel.window_stride)).cuda()
    lens = torch.from_numpy(rs.lens.astype(np.int32)).cuda()
    H = panel.hits_per_read
    d_ops = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    d_extra = torch.empty(max(64, n // 4) * 32, dtype=torch.uint8, device="cuda")
    d_hits = torch.empty(n * H * 24, dtype=torch.uint8, device="cuda")
    d_small = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_counts = torch.zeros(panel.counts_len, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.smx_batch_run_device(panel.handle, stream, windows.data_ptr(), lens.data_ptr(), n, d_ops.data_ptr(),
                                        d_extra.data_ptr(), max(64, n // 4), d_small.data_ptr(), d_counts.data_ptr(),
                                        d_hits.data_ptr(), None))
    torch.cuda.synchronize()
    fl = barcodes.DeviceFlank(panel, barcodes.DEFAULT_TABLE_CAPACITY)
    ms = []
    for _ in range(args.repeats + 1):
        fl.clear(stream)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fl.accumulate(stream, windows.data_ptr(), lens.data_ptr(), d_hits.data_ptr(), n)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[1:]
    keys, counts, counters = fl.read()
    fl.close()
    tot = counters.sum(axis=0).astype(np.int64)
    hits, counted = int(tot[0]), int(tot[5])
    floor_bytes = n * H * 24 + n * 4 + counted * 128
    t_floor = floor_bytes / HBM_PEAK
    print(f"[count] {n} reads x {H} (primer, end) records; {hits} primer hits: " +
          ", ".join(f"{name} {int(v)}" for name, v in zip(barcodes.COUNTERS[1:], tot[1:])))
    print(f"[count] {len(keys)} distinct flanks ({1000 * len(keys) / max(counted, 1):.0f} per 1000 counted hits), largest count "
          f"{int(counts.max()) if len(counts) else 0}, singletons {int((counts == 1).sum())}")
    print(f"[count] flank_count_kernel (HIP events): median {statistics.median(ms):.3f} ms, min {min(ms):.3f} ms over {len(ms)} launches "
          f"into an empty table of {barcodes.DEFAULT_TABLE_CAPACITY} slots")
    print(f"[count] must read: {n * H} hit records x 24 B + {n} lengths x 4 B + {counted} flanks x one 128 B line = "
          f"{floor_bytes / 1e6:.0f} MB = {floor_bytes / max(hits, 1):.0f} B per hit -> {t_floor * 1e3:.3f} ms at 8 TB/s; "
          f"kernel time = {min(ms) / (t_floor * 1e3):.1f} x that floor (the table's atomics are not in it)")
    info = {}
    report = barcodes.survey_table(panel, specs, keys, counts, counters, args.min_count, barcodes.DEFAULT_MAX_CANDIDATES, info)
    first = info["kernel_ms"]
    again = []
    for _ in range(args.repeats):
        barcodes.survey_table(panel, specs, keys, counts, counters, args.min_count, barcodes.DEFAULT_MAX_CANDIDATES, info)
        again.append(info["kernel_ms"])
    _bits, flen, _m, kprimer = barcodes.key_fields(keys)
    pairs = columns = 0
    for p, prim in enumerate(report):
        sel = kprimer == p
        pairs += int(sel.sum()) * len(prim["candidates"])
        columns += int(flen[sel].sum()) * len(prim["candidates"])
    t_valu = columns / 64 * INSTR_PER_COLUMN / VALU_PEAK
    print(f"[assign] {len(keys)} keys; candidates per primer " +
          ", ".join(f"{p['primer']} {len(p['candidates'])} ({sum(c['status'] == 'novel' for c in p['candidates'])} novel)" for p in report) +
          f"; {pairs / 1e6:.1f} M (key, candidate) pairs, {columns / 1e9:.2f} G columns")
    print(f"[assign] flank_assign_kernel (HIP events): first call {first:.3f} ms, then median {statistics.median(again):.3f} ms, "
          f"min {min(again):.3f} ms over {len(again)} calls")
    print(f"[assign] VALU minimum: columns x {INSTR_PER_COLUMN} instructions / 64 lanes over the issue peak = {t_valu * 1e3:.3f} ms; "
          f"kernel time = {min(again) / max(t_valu * 1e3, 1e-9):.1f} x that minimum")
    for prim in report:
        novel = [c for c in prim["candidates"] if c["status"] == "novel"][:3]
        print(f"[survey] {prim['primer']}: unexplained {prim['unexplained']}; first novel rows " +
              str([(c["barcode"], c["exact"], sum(c["support"])) for c in novel]))


if __name__ == "__main__":
    main()
