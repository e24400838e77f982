#!/usr/bin/env python3
"""Manual, longer-running parity fuzz (not collected by pytest): GPU records vs the oracle over many seeds, panel
shapes, flag sets and search lengths.  Run on a GPU box:  python tests/fuzz_parity.py [--seeds 8] [--reads 1200]
The synthetic panels are full barcode grids with one primer pair per pool; the scorer's rarer branches are reached by the
hand-written panels of tests/scorer_utils.py (multi, two_pairs, one_pair_sparse, wide, same_sequence): `--panel multi`
runs such a panel's constructed reads under every fuzz flag set.  The primer-search panels of tests/primer_utils.py (m22,
m31, m32, m33, m63, m64, m32_rev, m64_rev, deg5, c3_m33; c3 stays the synthetic panel) work the same way: `--panel m64`
builds the constructed reads for each flag set's search length."""
import argparse
import itertools
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from parity_utils import Both  # noqa: E402


def reads_of(rs, n, S):
    from parity_utils import reads_from_set
    return reads_from_set(rs, range(n), S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=6)
    ap.add_argument("--reads", type=int, default=1200)
    ap.add_argument("--trim", default=None, help="force this trim mode onto every flag set (e.g. tails)")
    ap.add_argument("--index-k", type=int, default=None, help="force this index edit distance onto every flag set")
    import scorer_utils as SU
    import primer_utils as PU
    primer_panels = [n for n in PU.PANELS if n != "c3"]
    ap.add_argument("--panel", default=None, choices=["c1", "c2", "c3"] + list(SU.PANELS) + primer_panels,
                    help="this panel only (default: c1, c2, c3 in rotation); a hand-written scorer panel of tests/scorer_utils.py "
                         "or a primer-search panel of tests/primer_utils.py runs its constructed reads (no seeds) under every "
                         "flag set")
    a = ap.parse_args()
    from specimux_amd import synth
    from parity_utils import FUZZ_FLAG_SETS
    flag_sets = [dict(f) for f in FUZZ_FLAG_SETS]
    if a.trim:
        flag_sets = [dict(f, trim=a.trim) for f in flag_sets if "trim" not in f]
    if a.index_k is not None:
        flag_sets = [dict(f, index_edit_distance=a.index_k) for f in flag_sets if "index_edit_distance" not in f]
    tmp = tempfile.mkdtemp(prefix="smx_fuzz_")
    if a.panel in SU.PANELS:
        pf, sf = SU.PANELS[a.panel].write(tmp)
        reads = SU.make_reads(SU.PANELS[a.panel])
        for flags in flag_sets:
            flags = {k: v for k, v in flags.items() if k not in ("error_rate", "n_frac")}
            both = Both(pf, sf, **flags)
            both.assert_hits_equal(reads[::10], f"{a.panel} {flags}")
            both.assert_ops_equal(reads, f"{a.panel} {flags}")
            print(f"ok {a.panel} {flags}  ({len(reads)} reads)", flush=True)
        print(f"fuzz parity OK: {a.panel}, {len(flag_sets)} flag sets")
        return
    if a.panel in primer_panels:
        pf, sf = PU.PANELS[a.panel]().write(tmp)
        for flags in flag_sets:
            flags = {k: v for k, v in flags.items() if k not in ("error_rate", "n_frac")}
            reads = PU.cell(a.panel, flags.get("search_len", 80)).reads
            both = Both(pf, sf, **flags)
            both.assert_hits_equal(reads, f"{a.panel} {flags}")
            both.assert_ops_equal(reads, f"{a.panel} {flags}")
            print(f"ok {a.panel} {flags}  ({len(reads)} reads)", flush=True)
        print(f"fuzz parity OK: {a.panel}, {len(flag_sets)} flag sets")
        return
    panels = {"c2": synth.panel_c2(), "c3": synth.panel_c3(), "c1": synth.panel_c1()}
    files = {}
    for name, pan in panels.items():
        d = os.path.join(tmp, name)
        os.makedirs(d)
        files[name] = pan.write(d)
    t0 = time.time()
    checked = 0
    for seed, (fi, flags) in itertools.product(range(a.seeds), enumerate(flag_sets)):
        name = a.panel or ("c2", "c3", "c1")[(seed + fi) % 3]
        pan, (pf, sf) = panels[name], files[name]
        flags = dict(flags)
        gen = {k: flags.pop(k) for k in ("error_rate", "n_frac") if k in flags}   # generator-only knobs
        S = flags.get("search_len", 80)
        rs = synth.make_reads(pan, a.reads, 9000 + 131 * seed + fi, search_len=S, windows_only=False, **gen)
        reads = reads_of(rs, a.reads, S)
        both = Both(pf, sf, **flags)
        both.assert_hits_equal(reads[:100], f"{name} seed {seed} {flags}")
        both.assert_ops_equal(reads, f"{name} seed {seed} {flags}")
        checked += len(reads)
        print(f"ok {name} seed {seed} {flags}  ({checked} reads, {time.time() - t0:.0f} s)", flush=True)
    print(f"fuzz parity OK: {checked} reads")


if __name__ == "__main__":
    main()
