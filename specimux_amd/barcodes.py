"""specimux-barcodes: which barcode sequences does a run hold next to a primer we recognise, and which of them does the
specimen sheet lack?

    python -m specimux_amd.barcodes primers.fasta specimens.txt reads.fastq[.gz]

The file is demultiplexed on the GPU for counting only (no output tree, no trace).  Behind every demux launch the flank
kernel (include/smx.h "Barcode survey", csrc/smx_flank.hip) cuts out, for every primer hit, the bases that sit where the
barcode should be, and counts them in a device table of (flank, count).  The host then takes, per primer,

  * the peaks: counts of the flanks' first `barcode length` bases;
  * the candidates: the primer's listed barcodes (canonical order) followed by the peaks the sheet does not list with at
    least --min-count exact copies (count descending, then sequence), --max-candidates in all;
  * one smx_flank_assign call that gives every distinct flank the candidate within the index distance that explains it
    best.  Listed barcodes come first, so they win every tie: the support of a novel candidate holds only flanks that no
    listed barcode explains as well.

A novel candidate with solid support is a barcode the run holds and the sheet lacks: a typo in an index, an index entered
reverse-complemented (`revcomp-of:`), the two index columns swapped (`other-primer:`), a well loaded from another plate.
Not in the reference.  Output is sorted: the same bytes from run to run and for any batch size."""
import argparse
import json
import logging
import sys

import numpy as np

logger = logging.getLogger("specimux_amd.barcodes")

COUNTERS = ("hits", "pruned", "short_read", "short_flank", "ambiguous", "counted")   # SMX_FLANK_* (include/smx.h)
LEN_SHIFT, MATCHED_SHIFT, PRIMER_SHIFT, MAX_W = 52, 57, 58, 26
DEFAULT_TABLE_CAPACITY = 1 << 22
DEFAULT_MIN_COUNT = 10          # a default, not a measured optimum
DEFAULT_MAX_CANDIDATES = 256
_RUN_FLAGS = {"--min-length", "--max-length", "--num-seqs", "--index-edit-distance", "--primer-edit-distance", "--search-len",
              "--disable-prefilter", "--disable-preorient"}


# ------------------------------------------------------------------------------------------------ keys
def encode_bases(seq):
    """ACGT string -> the 2-bit packing of a key's flank field (base t at bits [2t, 2t + 2)); None for any other letter."""
    bits = 0
    for t, ch in enumerate(seq):
        c = "ACGT".find(ch)
        if c < 0:
            return None
        bits |= c << (2 * t)
    return bits


def decode_bases(bits, n):
    bits = int(bits)
    return "".join("ACGT"[(bits >> (2 * t)) & 3] for t in range(n))


def key_fields(keys):
    """numpy uint64 keys -> (flank bits, flen, matched, primer) arrays."""
    keys = np.asarray(keys, dtype=np.uint64)
    bits = keys & np.uint64((1 << LEN_SHIFT) - 1)
    flen = ((keys >> np.uint64(LEN_SHIFT)) & np.uint64(31)).astype(np.int64)
    matched = ((keys >> np.uint64(MATCHED_SHIFT)) & np.uint64(1)).astype(np.int64)
    primer = (keys >> np.uint64(PRIMER_SHIFT)).astype(np.int64)
    return bits, flen, matched, primer


# ------------------------------------------------------------------------------------------------ device
class DeviceFlank:
    """smx_flank handle of one panel: the device table of flank keys and the per-primer counters."""

    def __init__(self, panel, capacity=DEFAULT_TABLE_CAPACITY):
        import ctypes as C
        from . import _lib
        self._lib, self.panel = _lib.load(), panel
        self.handle = C.c_void_p()
        _lib.check(self._lib.smx_flank_create(panel.handle, int(capacity), C.byref(self.handle)))
        self.slots = 8                      # smx_flank_create rounds the capacity up to a power of two, 8 at least
        while self.slots < int(capacity):
            self.slots <<= 1

    def accumulate(self, stream, d_windows, d_lens, d_hits, n):
        from . import _lib
        _lib.check(self._lib.smx_flank_accumulate_device(self.handle, stream, d_windows, d_lens, d_hits, int(n)))

    def read(self):
        """(keys, counts, counters [n_primers, 6]) numpy uint64; raises SmxError(ERR_OVERFLOW) when the table filled up.
        One call, one copy of the table: the host buffers are sized by the table's slots, which bound the distinct keys."""
        import ctypes as C
        from . import _lib
        n, dropped = C.c_uint32(), C.c_uint64()
        keys, counts = np.empty(self.slots, dtype=np.uint64), np.empty(self.slots, dtype=np.uint64)
        counters = np.zeros((len(self.panel.primers), len(COUNTERS)), dtype=np.uint64)
        _lib.check(self._lib.smx_flank_read(self.handle, _lib.ptr(keys), _lib.ptr(counts), self.slots, C.byref(n),
                                            _lib.ptr(counters), C.byref(dropped)))
        return keys[:n.value].copy(), counts[:n.value].copy(), counters

    def clear(self, stream=None):
        from . import _lib
        _lib.check(self._lib.smx_flank_clear(self.handle, stream))

    def close(self):
        if self.handle:
            self._lib.smx_flank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def assign(keys, candidates, k, info=None):
    """smx_flank_assign: keys (numpy uint64), candidates = [(primer index, end-string form)] -> (best, first, ntied) int32
    arrays; `first` indexes `candidates`.  info (dict) receives kernel_ms."""
    import ctypes as C
    from . import _lib
    lib = _lib.load()
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    text = "".join(seq for _p, seq in candidates).encode("ascii")
    off = np.zeros(len(candidates) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(seq) for _p, seq in candidates])
    primer = np.array([p for p, _seq in candidates] or [0], dtype=np.uint8)
    best, first, ntied = (np.full(max(1, len(keys)), -1, dtype=np.int32) for _ in range(3))
    ms = C.c_float(0)
    _lib.check(lib.smx_flank_assign(_lib.ptr(keys), len(keys), text, _lib.ptr(off), _lib.ptr(primer), len(candidates), int(k),
                                    _lib.ptr(best), _lib.ptr(first), _lib.ptr(ntied), C.byref(ms)))
    if info is not None:
        info["kernel_ms"] = float(ms.value)
    return best[:len(keys)], first[:len(keys)], ntied[:len(keys)]


def accumulate_batches(panel, flank, batches, n_slots=2, max_reads=None):
    """Window batches (windows, lens, ...) through the demux kernel and, behind each launch, the flank count kernel, on
    trace_stats.stream_batches' device-resident slots.  Returns the device counts vector."""
    from . import trace_stats

    def enqueue(s, sp, n):
        flank.accumulate(sp, s.d_windows.data_ptr(), s.d_lens.data_ptr(), s.d_hits.data_ptr(), n)

    return trace_stats.stream_batches(panel, batches, enqueue, n_slots=n_slots, max_reads=max_reads)


# ------------------------------------------------------------------------------------------------ the survey
def survey_table(panel, specimens, keys, counts, counters, min_count=DEFAULT_MIN_COUNT, max_candidates=DEFAULT_MAX_CANDIDATES,
                 info=None):
    """From a flank table to the report: [{primer, direction, counters, unexplained, candidates: [...]}] in panel order."""
    from .constants import Primer
    from .models import reverse_complement
    from .orchestration import edit_distance
    Lb, k = int(panel.desc.barcode_len_max), int(panel.desc.k_index)
    order = np.argsort(keys, kind="stable")            # the primer is the key's top field: sorted keys come grouped by primer
    keys, counts = np.asarray(keys, dtype=np.uint64)[order], np.asarray(counts, dtype=np.uint64)[order].astype(np.int64)
    bits, flen, matched, kprimer = key_fields(keys)
    prefix = bits & np.uint64((1 << (2 * Lb)) - 1)
    every_barcode = {b for p in panel.primers for b in p.barcodes}
    candidates, spans, peaks_of = [], [], []
    for p, primer in enumerate(panel.primers):
        sel = (kprimer == p) & (flen >= Lb)
        peak_bits, inverse = np.unique(prefix[sel], return_inverse=True)
        peak_count = np.bincount(inverse, weights=counts[sel], minlength=len(peak_bits)).astype(np.int64)
        peaks = dict(zip(peak_bits.tolist(), peak_count.tolist()))
        listed = [reverse_complement(b) for b in primer.barcodes]
        listed_bits = {encode_bases(s) for s in listed}
        novel = sorted(((n, decode_bases(b, Lb)) for b, n in peaks.items() if n >= min_count and b not in listed_bits),
                       key=lambda x: (-x[0], x[1]))
        novel = novel[:max(0, max_candidates - len(listed))]
        spans.append((len(candidates), len(listed), len(novel)))
        candidates += [(p, s) for s in listed] + [(p, s) for _n, s in novel]
        peaks_of.append(peaks)
    best, first, _ntied = assign(keys, candidates, k, info)
    # support[candidate][distance], and the part of it that came from keys without a panel barcode at their end
    support = np.zeros((len(candidates), k + 1), dtype=np.int64)
    unmatched = np.zeros(len(candidates), dtype=np.int64)
    ok = best >= 0
    np.add.at(support, (first[ok], best[ok]), counts[ok])
    np.add.at(unmatched, first[ok & (matched == 0)], counts[ok & (matched == 0)])
    report = []
    for p, primer in enumerate(panel.primers):
        c0, n_listed, n_novel = spans[p]
        fwd = primer.direction == Primer.FWD
        rows = []
        for c in range(c0, c0 + n_listed + n_novel):
            rc_form = candidates[c][1]
            barcode = reverse_complement(rc_form)
            known = c < c0 + n_listed
            eb = encode_bases(rc_form)
            row = {"barcode": barcode, "status": "known" if known else "novel", "specimens": 0,
                   "exact": int(peaks_of[p].get(eb, 0)) if eb is not None else 0,
                   "support": [int(x) for x in support[c]], "unmatched_support": int(unmatched[c]),
                   "nearest": None, "nearest_distance": None, "notes": []}
            if known:
                row["specimens"] = len(specimens.specimens_using_barcode(barcode, primer))
            else:
                if primer.barcodes:
                    d, _i, near = min((edit_distance(barcode, b), i, b) for i, b in enumerate(primer.barcodes))
                    row["nearest"], row["nearest_distance"] = near, int(d)
                if reverse_complement(barcode) in every_barcode:
                    row["notes"].append(f"revcomp-of:{reverse_complement(barcode)}")
                for other in panel.primers:
                    if other.direction != primer.direction and barcode in other.barcodes:
                        row["notes"].append(f"other-primer:{other.name}")
            rows.append(row)
        mine = kprimer == p
        report.append({"primer": primer.name, "direction": "forward" if fwd else "reverse",
                       "counters": {name: int(counters[p][i]) for i, name in enumerate(COUNTERS)},
                       "distinct_flanks": int(mine.sum()), "unexplained": int(counts[mine & ~ok].sum()), "candidates": rows})
    return report


def run_survey(primers, specimens, sequence_file, args, capacity=DEFAULT_TABLE_CAPACITY, batch_reads=None,
               min_count=DEFAULT_MIN_COUNT, max_candidates=DEFAULT_MAX_CANDIDATES):
    """The whole tool but its printing: returns the document --json writes."""
    from . import trace_stats
    trace_stats.refuse_distributed("specimux-barcodes")
    from .native_io import Reader
    batch_reads = int(batch_reads or trace_stats.RUN_BATCH_READS)
    ns, specs, _parameters, _prefilter, panel = trace_stats.load_run_panel(primers, specimens, sequence_file, args)
    reader = Reader(sequence_file)
    flank = None
    try:
        flank = DeviceFlank(panel, capacity)
        run_counts = accumulate_batches(panel, flank, trace_stats.file_batches(reader, panel, ns, batch_reads), n_slots=3,
                                        max_reads=batch_reads)
        keys, counts, counters = flank.read()
    finally:
        reader.close()
        if flank is not None:
            flank.close()
    info = {}
    report = survey_table(panel, specs, keys, counts, counters, min_count, max_candidates, info)
    return {"format": "specimux_amd barcode survey", "version": 1, "reads": int(run_counts[0]),
            "parameters": {"search_len": int(panel.search_len), "barcode_length": int(panel.desc.barcode_len_max),
                           "index_edit_distance": int(panel.desc.k_index), "min_count": int(min_count),
                           "max_candidates": int(max_candidates)},
            "distinct_flanks": int(len(keys)), "primers": report}


# ------------------------------------------------------------------------------------------------ output
def tsv_lines(doc):
    k = doc["parameters"]["index_edit_distance"]
    head = ["primer", "direction", "barcode", "status", "specimens", "exact"] + [f"support_d{d}" for d in range(k + 1)] + \
           ["support", "unmatched_support", "nearest", "nearest_distance", "notes"]
    yield "\t".join(head)
    for prim in doc["primers"]:
        for r in prim["candidates"]:
            yield "\t".join(str(x) for x in [prim["primer"], prim["direction"], r["barcode"], r["status"], r["specimens"], r["exact"]] +
                            r["support"] + [sum(r["support"]), r["unmatched_support"], r["nearest"] or "-",
                                            "-" if r["nearest_distance"] is None else r["nearest_distance"],
                                            ",".join(r["notes"]) or "-"])


def format_text(doc, top=None):
    par = doc["parameters"]
    k = par["index_edit_distance"]
    hits = sum(p["counters"]["hits"] for p in doc["primers"])
    lines = [f"Barcode survey: {doc['reads']:,} reads, {hits:,} primer hits, {doc['distinct_flanks']:,} distinct flanks",
             f"search length {par['search_len']}, barcode length {par['barcode_length']}, index distance {k}, "
             f"min count {par['min_count']}, max candidates {par['max_candidates']}"]
    for prim in doc["primers"]:
        c = prim["counters"]
        lines += ["", f"Primer {prim['primer']} ({prim['direction']})",
                  "  " + ", ".join(f"{name} {c[name]:,}" for name in COUNTERS) +
                  f"; {prim['distinct_flanks']:,} distinct flanks; counted hits no candidate explains: {prim['unexplained']:,}"]
        rows = sorted(prim["candidates"], key=lambda r: (-r["exact"], r["barcode"]))
        shown = rows if top is None else rows[:max(0, top)]
        w = max([len(r["barcode"]) for r in shown] + [7])
        lines.append(f"  {'barcode':<{w}}  {'status':<10} {'exact':>9} " + " ".join(f"{'d=' + str(d):>8}" for d in range(k + 1)) +
                     f" {'unmatched':>10}  notes")
        for r in shown:
            status = f"known({r['specimens']})" if r["status"] == "known" else "novel"
            notes = list(r["notes"])
            if r["nearest"] is not None:
                notes.insert(0, f"nearest:{r['nearest']}({r['nearest_distance']})")
            lines.append(f"  {r['barcode']:<{w}}  {status:<10} {r['exact']:>9,} " + " ".join(f"{x:>8,}" for x in r["support"]) +
                         f" {r['unmatched_support']:>10,}  {' '.join(notes)}".rstrip())
        if len(shown) < len(rows):
            lines.append(f"  ... {len(rows) - len(shown)} more candidate(s): --top, --report, --json")
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ command line
def build_parser():
    parser = argparse.ArgumentParser(
        prog="specimux-barcodes", description="Find the barcodes a run holds next to its primers and the specimen sheet lacks")
    parser.add_argument("primer_file", help="Fasta file containing primer information")
    parser.add_argument("specimen_file", help="TSV file containing specimen mapping with barcodes and primers")
    parser.add_argument("sequence_file", help="Sequence file in Fasta or Fastq format, gzipped or plain text")
    parser.add_argument("--min-count", type=int, default=DEFAULT_MIN_COUNT,
                        help=f"exact copies an unlisted sequence needs to become a candidate (default {DEFAULT_MIN_COUNT})")
    parser.add_argument("--max-candidates", type=int, default=DEFAULT_MAX_CANDIDATES,
                        help=f"candidates per primer, listed barcodes included (default {DEFAULT_MAX_CANDIDATES})")
    parser.add_argument("--top", type=int, default=None, metavar="N", help="print only the N candidates with the most exact copies per primer")
    parser.add_argument("--report", metavar="FILE.tsv", help="write one row per candidate")
    parser.add_argument("--json", metavar="FILE", help="write the whole survey as JSON")
    parser.add_argument("--table-capacity", type=int, default=DEFAULT_TABLE_CAPACITY,
                        help=f"slots of the device table of distinct flanks (default {DEFAULT_TABLE_CAPACITY}); the run fails if it fills up")
    from . import cli
    run = parser.add_argument_group("the matching flags of specimux")
    for flags, kwargs in cli._OPTIONS:
        if _RUN_FLAGS & set(flags):
            run.add_argument(*flags, **kwargs)
    run.add_argument("--start-seq", type=int, default=None, help="first sequence to read, 1-based (as -n START,NUM)")
    return parser


def main(argv=None):
    """argv without the program name; returns the exit status.  Messages go to stderr as "LEVEL - text"."""
    handler = logging.StreamHandler(sys.stderr)
    handler.setFormatter(logging.Formatter("%(levelname)s - %(message)s"))
    logger.addHandler(handler)
    logger.setLevel(logging.INFO)
    propagate, logger.propagate = logger.propagate, False
    try:
        return _main(sys.argv[1:] if argv is None else list(argv))
    finally:
        logger.removeHandler(handler)
        logger.propagate = propagate


def _main(argv):
    parser = build_parser()
    args = parser.parse_args(argv)
    from . import cli
    start = args.start_seq
    args = cli.split_num_seqs(parser, args)
    if start is not None:
        args.start_seq = start
    if args.min_count < 1 or args.max_candidates < 1 or args.table_capacity < 1:
        parser.error("--min-count, --max-candidates and --table-capacity must be positive")
    try:
        doc = run_survey(args.primer_file, args.specimen_file, args.sequence_file, args, capacity=args.table_capacity,
                         min_count=args.min_count, max_candidates=args.max_candidates)
        if args.json:
            with open(args.json, "w") as fh:
                json.dump(doc, fh, indent=1, sort_keys=True)
                fh.write("\n")
        if args.report:
            with open(args.report, "w") as fh:
                fh.write("\n".join(tsv_lines(doc)) + "\n")
        print(format_text(doc, args.top))
    except Exception as e:
        logger.error(f"Error: {e}")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
