"""specimux-stats: match statistics of a run ("pool -> primer pair -> outcome" tables, Sankey flow data).

Reference: src/specimux/trace_stats.py -- same command line, dimension names, validation messages, hierarchical text and
Sankey JSON keys.  Two sources here:

  * a trace directory (`specimux -d` output, specimux_amd/trace.py writes the same TSV), as in the reference;
  * `--from-run PRIMERS SPECIMENS SEQUENCE_FILE`: the file is demultiplexed on the GPU for counting only -- no output
    tree, no trace -- and the rows are counted on the device (include/smx.h "Match statistics", csrc/smx_stats.hip).

Both produce one thing, a StatsTable: {(the eleven stored dimensions, first candidate of its read): count}.  Every
report (tree, Sankey nodes and links, totals, `--count-by sequences` = the rows with the first-candidate bit) is computed
from that table, never from a list of per-candidate objects, so a 50 M-read run is summarised from a few thousand rows.
`--save-table` / `--table` store and reload it (JSON): count once, query many times.

`candidate_match_id` and `sequence_id` are per-row identities, not table columns: they are listed where the reference
lists them and rejected as grouping dimensions.  Sankey links are emitted sorted by (source, target); the reference emits
them in order of first appearance in the data, which a table of counts does not know.

Three properties of the reference tool are reproduced on purpose: with `--dereplicate best` a dereplicated full match
has resolution and outcome `unknown` (the reference logs no SPECIMEN_RESOLVED event for it); the first
SPECIMEN_RESOLVED event of a read is applied to all its surviving candidates; `selection_strategy` is only ever `none`
or `discarded` (nothing in the reference emits MATCH_SELECTED)."""
import argparse
import csv
import glob
import json
import logging
import os
import sys
from collections import Counter, OrderedDict
from pathlib import Path

logger = logging.getLogger("specimux_amd.trace_stats")

STORED = ("orientation", "forward_primer", "reverse_primer", "pool", "forward_barcode", "reverse_barcode", "match_type",
          "resolution_type", "outcome", "selection_strategy", "discard_reason")
_DEFAULT_ROW = ("unknown", "none", "none", "none", "none", "none", "none", "unknown", "unknown", "none", "none")
_IX = {name: i for i, name in enumerate(STORED)}
IDENTITIES = ("candidate_match_id", "sequence_id")

COMPUTED = {
    "forward_barcode_matched": lambda r: r[_IX["forward_barcode"]] != "none",
    "reverse_barcode_matched": lambda r: r[_IX["reverse_barcode"]] != "none",
    "specimen_matched": lambda r: r[_IX["outcome"]] == "matched",
    "barcode_count": lambda r: (r[_IX["forward_barcode"]] != "none") + (r[_IX["reverse_barcode"]] != "none"),
    "primer_pair": lambda r: f"{r[_IX['forward_primer']]}-{r[_IX['reverse_primer']]}",
    "barcode_pair": lambda r: f"{r[_IX['forward_barcode']]}-{r[_IX['reverse_barcode']]}",
    "outcome_detailed": lambda r: (f"discarded_{r[_IX['discard_reason']]}"
                                   if r[_IX["outcome"]] == "discarded" and r[_IX["discard_reason"]] != "none"
                                   else r[_IX["outcome"]]),
}
ALL_DIMENSIONS = sorted(STORED + tuple(COMPUTED) + IDENTITIES)
COUNT_MODES = ("candidate_matches", "sequences")


def dimension_value(row, name):
    return row[_IX[name]] if name in _IX else COMPUTED[name](row)


class StatsTable:
    """{(row of the eleven stored dimensions, is first candidate of its read): count}."""

    def __init__(self):
        self.counts = Counter()
        self.host_replayed = 0    # --from-run: reads whose rows the host had to derive (trim-to-empty primary record)

    def add(self, row, first, n=1):
        self.counts[(tuple(row), bool(first))] += n

    def __eq__(self, other):
        return isinstance(other, StatsTable) and +self.counts == +other.counts

    def total(self, count_by="candidate_matches"):
        return sum(n for (_r, first), n in self.counts.items() if first or count_by != "sequences")

    def rows(self, count_by):
        """(row, count) pairs of the counting mode; equal rows are not merged (the aggregator sums anyway)."""
        for (row, first), n in self.counts.items():
            if n and (first or count_by != "sequences"):
                yield row, n

    # ---- JSON
    def to_json(self):
        return {"format": "specimux_amd stats table", "version": 1, "dimensions": list(STORED),
                "host_replayed": self.host_replayed,
                "rows": [list(row) + [first, n] for (row, first), n in sorted(self.counts.items()) if n]}

    @classmethod
    def from_json(cls, doc):
        if doc.get("format") != "specimux_amd stats table" or doc.get("dimensions") != list(STORED):
            raise ValueError("not a stats table written by --save-table")
        t = cls()
        t.host_replayed = int(doc.get("host_replayed", 0))
        for rec in doc["rows"]:
            t.add(rec[:len(STORED)], rec[len(STORED)], int(rec[len(STORED) + 1]))
        return t

    def merge(self, other):
        """Add another table's counts and host_replayed to this one (rows are names, so tables of different panel builds,
        files or ranks add up).  Returns self."""
        self.counts.update(other.counts)
        self.host_replayed += other.host_replayed
        return self

    def save(self, path):
        """Atomic: the table goes to a temporary file in the same directory, which then replaces `path`; a reader (or a
        `--table` query during a live run) never sees half a table, and a failed write leaves the previous file."""
        path = os.fspath(path)
        tmp = f"{path}.tmp{os.getpid()}"
        try:
            with open(tmp, "w") as fh:
                json.dump(self.to_json(), fh)
            os.replace(tmp, path)
        except BaseException:
            try:
                os.unlink(tmp)
            except OSError:
                pass
            raise

    @classmethod
    def load(cls, path):
        with open(path) as fh:
            return cls.from_json(json.load(fh))


# ------------------------------------------------------------------------------------------------ source 1: trace TSV
# column counts below which the reference's parser leaves an event without its fields (trace_stats.py:176-239)
_FIELDS = {"ORIENTATION_DETECTED": (9, ("orientation",)),
           "PRIMER_MATCHED": (13, ("candidate_match_id", "match_type", "forward_primer", "reverse_primer", None, None, "pool")),
           "BARCODE_MATCHED": (13, ("candidate_match_id", "match_type", "forward_barcode", "reverse_barcode")),
           "MATCH_SELECTED": (12, ("selection_strategy", "forward_primer", "reverse_primer", "forward_barcode", "reverse_barcode")),
           "SPECIMEN_RESOLVED": (12, (None, "resolution_type")),
           "MATCH_DISCARDED": (12, ("candidate_match_id", None, None, None, None, None, "discard_reason"))}
_OUTCOME = {"full_match": "matched", "partial_forward": "partial", "partial_reverse": "partial"}


def _sequence_rows(events):
    """The rows of one read from its events in file order: [(row, first)]."""
    orientation = next((e.get("orientation", "unknown") for e in events if e["type"] == "ORIENTATION_DETECTED"), "unknown")
    primer_events = [e for e in events if e["type"] == "PRIMER_MATCHED"]
    if not primer_events:
        return [((orientation,) + _DEFAULT_ROW[1:], True)]
    resolved = next((e for e in events if e["type"] == "SPECIMEN_RESOLVED"), None)
    out = []
    for n, pe in enumerate(primer_events):
        cid = pe.get("candidate_match_id")
        row = dict(zip(STORED, _DEFAULT_ROW))
        row["orientation"] = orientation
        for k in ("forward_primer", "reverse_primer", "pool", "match_type"):
            row[k] = pe.get(k, "none")
        be = next((e for e in events if e["type"] == "BARCODE_MATCHED" and e.get("candidate_match_id") == cid), None)
        if be is not None:
            row["forward_barcode"] = be.get("forward_barcode", "none")
            row["reverse_barcode"] = be.get("reverse_barcode", "none")
            if "match_type" in be:
                row["match_type"] = be["match_type"]
        de = next((e for e in events if e["type"] == "MATCH_DISCARDED" and e.get("candidate_match_id") == cid), None)
        if de is not None:
            row["outcome"] = row["selection_strategy"] = "discarded"
            row["discard_reason"] = de.get("discard_reason", "unknown")
        else:
            for se in events:
                if se["type"] == "MATCH_SELECTED" and all(
                        row[k] == se.get(k, "none") for k in ("forward_primer", "reverse_primer", "forward_barcode", "reverse_barcode")):
                    row["selection_strategy"] = se.get("selection_strategy", "unknown")
                    break
            if resolved is not None:
                row["resolution_type"] = resolved.get("resolution_type", "unknown")
                row["outcome"] = _OUTCOME.get(row["resolution_type"], "unknown")
        out.append((tuple(row[k] for k in STORED), n == 0))
    return out


def table_from_rows(rows):
    """rows: iterables of TSV columns [timestamp, worker_id, event_seq, sequence_id, event_type, fields...]."""
    by_seq = OrderedDict()
    for cols in rows:
        if len(cols) < 5:
            continue
        ev = {"type": cols[4]}
        need, names = _FIELDS.get(cols[4], (0, ()))
        if names and len(cols) >= need:
            for name, value in zip(names, cols[5:]):
                if name:
                    ev[name] = value
        by_seq.setdefault(cols[3], []).append(ev)
    table = StatsTable()
    for events in by_seq.values():
        for row, first in _sequence_rows(events):
            table.add(row, first)
    return table


def _file_rows(path):
    with open(path, newline="") as fh:
        reader = csv.reader(fh, delimiter="\t")
        if next(reader, None) is None:
            logger.warning(f"Empty trace file: {path}")
            return
        yield from reader


def table_from_trace_dir(trace_directory):
    files = glob.glob(str(Path(trace_directory) / "specimux_trace_*.tsv"))
    if not files:
        raise ValueError(f"No trace files found in {trace_directory}")
    logger.info(f"Found {len(files)} trace files")

    def every():
        for f in files:
            yield from _file_rows(f)
    return table_from_rows(every())


# ------------------------------------------------------------------------------------------------ the aggregator
class StatsAggregator:
    """Trees and Sankey data over a StatsTable for any list of dimensions."""

    def __init__(self, table: StatsTable):
        self.table = table
        self.available_dimensions = list(ALL_DIMENSIONS) if table.total() else []

    def _validate(self, dimensions, count_by):
        invalid = [d for d in dimensions if d not in self.available_dimensions]
        if invalid:
            raise ValueError(f"Invalid dimensions: {invalid}. Available: {self.available_dimensions}")
        ids = [d for d in dimensions if d in IDENTITIES]
        if ids:
            raise ValueError(f"{ids} identify single rows and are not kept in a table of counts: they cannot be grouped by")
        if count_by not in COUNT_MODES:
            raise ValueError(f"count_by must be 'candidate_matches' or 'sequences', got: {count_by}")

    def _grouped(self, dimensions, count_by):
        """{tuple of dimension values: count}"""
        out = Counter()
        for row, n in self.table.rows(count_by):
            out[tuple(dimension_value(row, d) for d in dimensions)] += n
        return out

    def get_hierarchical_stats(self, dimensions, count_by="candidate_matches"):
        self._validate(dimensions, count_by)
        tree = {}
        for values, n in self._grouped(dimensions, count_by).items():
            node = tree
            for v in values[:-1]:
                node = node.setdefault(v, {})
            node[values[-1]] = node.get(values[-1], 0) + n
        return {"dimensions": list(dimensions), "count_by": count_by, "total_count": self.table.total(count_by), "data": tree}

    def get_sankey_data(self, dimensions, count_by="candidate_matches"):
        self._validate(dimensions, count_by)
        grouped = self._grouped(dimensions, count_by)
        nodes = []
        for layer, dim in enumerate(dimensions):
            for value in sorted({values[layer] for values in grouped}):
                nodes.append({"id": f"{dim}_{value}", "label": f"{dim}: {value}", "layer": layer, "dimension": dim, "value": value})
        known = {node["id"] for node in nodes}
        links = []
        for i in range(len(dimensions) - 1):
            flows = Counter()
            for values, n in grouped.items():
                flows[(f"{dimensions[i]}_{values[i]}", f"{dimensions[i + 1]}_{values[i + 1]}")] += n
            links += [{"source": src, "target": dst, "value": n} for (src, dst), n in flows.items() if src in known and dst in known]
        links.sort(key=lambda link: (link["source"], link["target"]))
        return {"dimensions": list(dimensions), "count_by": count_by, "total_count": self.table.total(count_by),
                "nodes": nodes, "links": links}


def _subtotal(node):
    return node if isinstance(node, int) else sum(_subtotal(v) for v in node.values())


def format_hierarchical_output(stats, indent="     "):
    total = stats["total_count"]
    width = len(f"{total:,}")
    dims = stats["dimensions"]
    lines = [f"Hierarchical Statistics: {' → '.join(dims)}", f"Count by: {stats['count_by']}", f"Total: {total:,}", ""]

    def level(node, depth, parent_total):
        for key in sorted(node, key=str):
            sub = _subtotal(node[key])
            pct = (sub / parent_total * 100) if parent_total > 0 else 0
            lines.append(f"{indent * depth}{pct:5.1f}% {sub:{width},} {key} ({dims[depth]})")
            if not isinstance(node[key], int):
                level(node[key], depth + 1, sub)

    level(stats["data"], 0, total)
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ source 2: a run on the GPU
_ORI = ("unknown", "forward", "reverse")
# SMX_STATS_CLASS_* -> (resolution_type, outcome, selection_strategy, discard_reason)
_CLASS = (("unknown", "unknown", "none", "none"), ("full_match", "matched", "none", "none"),
          ("partial_forward", "partial", "none", "none"), ("partial_reverse", "partial", "none", "none"),
          ("multiple_specimens", "unknown", "none", "none"), ("unknown", "discarded", "discarded", "lower_score"))


def decode_key(panel, key):
    """One packed key (include/smx.h, "Match statistics") -> (row of the stored dimensions, first)."""
    key = int(key)
    ori, pair1 = key & 3, (key >> 2) & 0xfff
    p1, p2 = (key >> 14) & 1, (key >> 15) & 1
    b1, b2 = (key >> 16) & 0x1fff, (key >> 29) & 0x1fff
    cls, first = (key >> 42) & 7, (key >> 45) & 1
    if pair1 == 0:
        return (_ORI[ori],) + _DEFAULT_ROW[1:], bool(first)
    f, r, pool = panel.pairs[pair1 - 1]
    res, outcome, strategy, reason = _CLASS[cls]
    mt = "both" if b1 and b2 else "forward_only" if b1 else "reverse_only" if b2 else "none"
    row = (_ORI[ori], panel.primer_names[f] if p1 else "none", panel.primer_names[r] if p2 else "none",
           panel.pools[pool] if pool >= 0 else "none", panel.barcodes[b1 - 1] if b1 else "none",
           panel.barcodes[b2 - 1] if b2 else "none", mt, res, outcome, strategy, reason)
    return row, bool(first)


def table_from_keys(panel, keys, counts, table=None):
    table = table or StatsTable()
    for k, n in zip(keys, counts):
        row, first = decode_key(panel, k)
        table.add(row, first, int(n))
    return table


class _ResolvedTrace:
    """A trace logger that keeps the SPECIMEN_RESOLVED types of one read and ignores the rest."""
    verbosity = 0

    def __init__(self):
        self.resolved = []

    def log_specimen_resolved(self, _sid, _match, _specimen, resolution_type, _pool):
        self.resolved.append(resolution_type)

    def __getattr__(self, name):
        if name.startswith("log_"):
            return lambda *a, **k: None
        raise AttributeError(name)


class HostReplay:
    """The reads the device cannot decide (their primary record is a trim-to-empty fallback, which has lost the
    resolution that was asked for): their rows come from the existing replay of the reference's control flow
    (trace.BatchReplayer) over the per-barcode hit dump of just those reads.  `panel`: a CompiledPanel, or any object with
    its primers / primer_names / barcodes / pools / pairs tables."""

    def __init__(self, panel, parameters, specimens, args, prefilter_on):
        from .constants import Primer
        from .trace import BatchReplayer
        self.panel = panel
        self.preorient = bool(parameters.preorient)
        self.pdir = [0 if p.direction == Primer.FWD else 1 for p in panel.primers]
        self.replayer = BatchReplayer(panel, parameters, specimens, args, prefilter_on)

    def keys_of_read(self, seq, hits, bdist, filtered=False):
        """Packed keys of one read from its hit records and per-barcode distances (smx_hit[2 * NP], int8[2 * NP][maxB])."""
        from .io_utils import SeqRecord
        tl = _ResolvedTrace()
        if not filtered:
            self.replayer.replay(tl, SeqRecord(seq, "r", "r", None), seq, "r", hits, bdist, None)
        res = tl.resolved[0] if tl.resolved else "unknown"
        cls = {"full_match": 1, "partial_forward": 2, "partial_reverse": 3, "multiple_specimens": 4}.get(res, 0)
        return _keys_of_read(self.panel.pairs, self.pdir, self.preorient, hits, filtered, cls)

    def close(self):
        """Nothing of its own on the device (the replay runs through the panel): drop the references."""
        self.replayer = None

    def add_rows(self, table, windows, lens, seqs):
        """windows / lens: the packed windows of the reads (numpy), seqs: their sequences (only the lengths matter)."""
        import numpy as np
        from . import _lib
        ops, _extra, _counts, hits, bdist = self.panel.run(np.ascontiguousarray(windows), np.ascontiguousarray(lens), want_hits=True)
        for i, seq in enumerate(seqs):
            for key in self.keys_of_read(seq, hits[i], bdist[i], int(ops["rtype"][i]) == _lib.R_FILTERED):
                row, first = decode_key(self.panel, key)
                table.add(row, first)
            table.host_replayed += 1


def _keys_of_read(pairs, pdir, preorient, hits, filtered, cls):
    """The rule of csrc/smx_stats_core.h (stats_read) for one read whose resolution class is already known: the host
    copy, used only for the host-replayed reads."""
    if filtered:
        return [1 << 45]
    ori = 0
    if preorient:
        f = r = 0
        for p, d in enumerate(pdir):
            va, vb = int(hits[2 * p]["flags"]) & 1, int(hits[2 * p + 1]["flags"]) & 1
            if d == 0:
                f, r = f + va, r + vb
            else:
                f, r = f + vb, r + va
        ori = 1 if (f > 0 and r == 0) else 2 if (r > 0 and f == 0) else 0
    cands = []
    for pi, (fw, rv, _pool) in enumerate(pairs):
        for o in (0, 1):
            if (o == 0 and ori == 2) or (o == 1 and ori == 1):
                continue
            h1, h2 = hits[2 * fw + o], hits[2 * rv + (1 - o)]
            p1, p2 = bool(h1["pdist"] >= 0), bool(h2["pdist"] >= 0)
            if not (p1 or p2):
                continue
            b1 = int(h1["first_tied"]) + 1 if p1 and h1["bbest"] >= 0 else 0
            b2 = int(h2["first_tied"]) + 1 if p2 and h2["bbest"] >= 0 else 0
            nb = (b1 > 0) + (b2 > 0)
            score = 5 if p1 and p2 and nb == 2 else 4 if p1 and p2 and nb else 3 if nb else 2 if p1 and p2 else 1
            cands.append((score, ori | (pi + 1) << 2 | int(p1) << 14 | int(p2) << 15 | b1 << 16 | b2 << 29))
    if not cands:
        return [ori | 1 << 45]
    best = max(s for s, _k in cands)
    return [k | (cls if s == best else 5) << 42 | (1 << 45 if n == 0 else 0) for n, (s, k) in enumerate(cands)]


class DeviceStats:
    """smx_stats handle of one panel."""

    def __init__(self, panel, capacity):
        import ctypes as C
        from . import _lib
        self._lib, self.panel = _lib.load(), panel
        self.handle = C.c_void_p()
        _lib.check(self._lib.smx_stats_create(panel.handle, int(capacity), C.byref(self.handle)))

    def accumulate(self, stream, d_hits, d_ops, n, d_fallback=None, fallback_cap=0, d_n_fallback=None):
        from . import _lib
        _lib.check(self._lib.smx_stats_accumulate_device(self.handle, stream, d_hits, d_ops, int(n), d_fallback,
                                                         int(fallback_cap), d_n_fallback))

    def read(self):
        """(keys, counts) numpy uint64; raises SmxError(ERR_OVERFLOW) when the table filled up."""
        import ctypes as C
        import numpy as np
        from . import _lib
        n, dropped = C.c_uint32(), C.c_uint64()
        rc = self._lib.smx_stats_read(self.handle, None, None, 0, C.byref(n), C.byref(dropped))
        if rc != _lib.OK and not (rc == _lib.ERR_ARG and n.value):
            _lib.check(rc)
        keys, counts = np.zeros(max(1, n.value), dtype=np.uint64), np.zeros(max(1, n.value), dtype=np.uint64)
        _lib.check(self._lib.smx_stats_read(self.handle, _lib.ptr(keys), _lib.ptr(counts), len(keys), C.byref(n), C.byref(dropped)))
        return keys[:n.value], counts[:n.value]

    def clear(self, stream=None):
        from . import _lib
        _lib.check(self._lib.smx_stats_clear(self.handle, stream))

    def close(self):
        if self.handle:
            self._lib.smx_stats_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StatsTableFull(RuntimeError):
    """The device table of a counting run filled up.  `result`: what the run returns otherwise (its tree is complete)."""
    result = None


class RunStats:
    """What pipeline.run_streaming(..., match_stats=) counts a run into: the device table of the panel (`device`), the host
    replay for the reads the device cannot decide (`replay`) and the host table of names (`table`) that receives the
    replayed rows during the run and the decoded device table at its end."""

    def __init__(self, panel, parameters, specimens, args, prefilter_on, capacity=None):
        self.panel = panel
        self.capacity = int(capacity or DEFAULT_TABLE_CAPACITY)
        self.device = DeviceStats(panel, self.capacity)
        self.replay = HostReplay(panel, parameters, specimens, args, prefilter_on)
        self.table = StatsTable()

    def reset(self):
        """Empty device table (asynchronous: Lane.attach_stats waits for it) and a new host table, for the next run."""
        self.device.clear()
        self.table = StatsTable()

    def collect(self):
        """End of a run: the device table, decoded to names, is added to the host table."""
        from . import _lib
        try:
            keys, cnts = self.device.read()
        except _lib.SmxError as e:
            if e.code != _lib.ERR_OVERFLOW:
                raise
            raise StatsTableFull(f"the statistics table ({self.capacity} slots asked for) filled up, nothing is lost but the "
                                 f"table: run again with a larger --stats-table-capacity") from e
        table_from_keys(self.panel, keys, cnts, self.table)
        return self.table

    def summary(self):
        return (f"{self.table.total('sequences'):,} reads counted, {len(self.table.counts):,} distinct rows, "
                f"host_replayed {self.table.host_replayed}")

    def close(self):
        self.replay.close()
        self.device.close()


def rank_table_path(path, rank):
    return f"{os.fspath(path)}.rank{rank}"


def merge_rank_tables(path, world):
    """The tables `path`.rank0 .. `path`.rank<world-1> that the ranks of a sharded run saved, merged into `path`; the rank
    files are removed.  A missing or unreadable rank file is an error: no `path` is written (the others are still removed)."""
    parts = [rank_table_path(path, k) for k in range(world)]
    try:
        table = StatsTable()
        for k, part in enumerate(parts):
            if not os.path.exists(part):
                raise FileNotFoundError(f"rank {k} left no stats table ({part}): {os.fspath(path)} is not written")
            table.merge(StatsTable.load(part))
        table.save(path)
        return table
    finally:
        for part in parts:
            try:
                os.unlink(part)
            except OSError:
                pass


class _Slot:
    """Device and pinned host buffers of one batch in flight, on a stream of its own."""

    def __init__(self, torch, panel, max_reads, extra_cap, fallback_cap):
        dev = torch.device("cuda", torch.cuda.current_device())
        u8 = dict(dtype=torch.uint8, device=dev)
        self.stream = torch.cuda.Stream()
        self.h_windows = torch.empty((max_reads, panel.window_stride), dtype=torch.uint8).pin_memory()
        self.h_lens = torch.empty(max_reads, dtype=torch.int32).pin_memory()
        self.d_windows = torch.empty((max_reads, panel.window_stride), **u8)
        self.d_lens = torch.empty(max_reads, dtype=torch.int32, device=dev)
        self.d_ops = torch.empty(max_reads * 32, **u8)
        self.d_extra = torch.empty(max(1, extra_cap) * 32, **u8)
        self.d_hits = torch.empty(max_reads * panel.hits_per_read * 24, **u8)
        self.d_small = torch.zeros(2 + fallback_cap, dtype=torch.int32, device=dev)   # n_extra, n_fallback, fallback indices
        self.h_small = torch.zeros(2 + fallback_cap, dtype=torch.int32).pin_memory()
        self.extra_cap, self.fallback_cap = extra_cap, fallback_cap
        self.batch, self.n = None, 0


def stream_batches(panel, batches, enqueue, retired=None, n_slots=2, extra_cap=None, max_reads=None, fallback_cap=0):
    """Run window batches -- an iterable of (windows uint8 [n, stride], lens int32 [n], anything) -- through the demux kernel
    with the lean hit dump, everything resident on the device, `n_slots` batches in flight on as many streams.
    enqueue(slot, stream pointer, n) is called inside the slot's stream right behind the demux launch, for the kernel that
    consumes what the launch left in the slot (its windows, lengths, records and hits); retired(slot) when the slot's
    batch is complete and slot.h_small holds its counters.  max_reads: the largest batch (None: `batches` is a list and is
    measured); fallback_cap: int32 words behind the two counters of slot.d_small (None: one per read).  Only the small
    counters of a batch come back; an extra-record buffer that overflows is no reason to rerun a batch, counting needs
    the primary records only.  Returns the device counts vector (numpy uint64)."""
    import numpy as np
    import torch
    from . import _lib
    lib = _lib.load()
    if max_reads is None:
        batches = list(batches)
        max_reads = max([len(b[1]) for b in batches] + [1])
    slots = [_Slot(torch, panel, max_reads, extra_cap if extra_cap is not None else max(64, max_reads // 4),
                   max_reads if fallback_cap is None else fallback_cap) for _ in range(max(1, n_slots))]
    d_counts = torch.zeros(panel.counts_len, dtype=torch.int64, device=slots[0].d_ops.device)
    torch.cuda.synchronize()
    panel.set_streams(len(slots))

    def retire(s):
        if s.batch is None:
            return
        s.stream.synchronize()
        if retired is not None:
            retired(s)
        s.batch = None

    try:
        for bi, batch in enumerate(batches):
            windows, lens = batch[0], batch[1]
            s = slots[bi % len(slots)]
            retire(s)
            n = len(lens)
            if n == 0:
                continue
            s.h_windows[:n].numpy()[...] = windows
            s.h_lens[:n].numpy()[...] = lens
            with torch.cuda.stream(s.stream):
                s.d_windows[:n].copy_(s.h_windows[:n], non_blocking=True)
                s.d_lens[:n].copy_(s.h_lens[:n], non_blocking=True)
                sp = s.stream.cuda_stream
                _lib.check(lib.smx_batch_run_device(panel.handle, sp, s.d_windows.data_ptr(), s.d_lens.data_ptr(), n,
                                                    s.d_ops.data_ptr(), s.d_extra.data_ptr(), s.extra_cap,
                                                    s.d_small.data_ptr(), d_counts.data_ptr(), s.d_hits.data_ptr(), None))
                enqueue(s, sp, n)
                s.h_small.copy_(s.d_small, non_blocking=True)
            s.batch = batch
        for s in slots:
            retire(s)
        torch.cuda.synchronize()
    finally:
        panel.set_streams(1)
    return d_counts.cpu().numpy().astype(np.uint64)


def accumulate_batches(panel, stats, batches, replay=None, table=None, n_slots=2, extra_cap=None, max_reads=None):
    """stream_batches with the statistics kernel behind every demux launch: batches of (windows, lens, sequences by index
    or None).  Only the two counters and the fallback indices of a batch come back.  Rows of host-replayed reads go to
    `table`.  Returns the device counts vector (numpy uint64)."""
    import numpy as np

    def enqueue(s, sp, n):
        stats.accumulate(sp, s.d_hits.data_ptr(), s.d_ops.data_ptr(), n, s.d_small.data_ptr() + 8, s.fallback_cap,
                         s.d_small.data_ptr() + 4)

    def retired(s):
        n_fb = int(s.h_small[1])
        if n_fb:
            if replay is None or table is None:
                raise RuntimeError(f"{n_fb} read(s) need the host replay (trim-to-empty primary record) and no replayer was given")
            idx = np.sort(s.h_small[2:2 + n_fb].numpy().astype(np.int64))
            windows, lens, seqs = s.batch
            seqs = [seqs[i] for i in idx] if seqs is not None else ["N" * int(lens[i]) for i in idx]
            replay.add_rows(table, windows[idx], lens[idx], seqs)

    return stream_batches(panel, batches, enqueue, retired, n_slots=n_slots, extra_cap=extra_cap, max_reads=max_reads,
                          fallback_cap=None)


DEFAULT_TABLE_CAPACITY = 1 << 16
RUN_BATCH_READS = 1 << 18


_RUN_FLAGS = {"--min-length", "--max-length", "--num-seqs", "--index-edit-distance", "--primer-edit-distance", "--search-len",
              "--trim", "--dereplicate", "--disable-prefilter", "--disable-preorient"}


def refuse_distributed(tool):
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise RuntimeError(f"{tool} counts in a single process; it cannot run under torch.distributed.run "
                           f"(WORLD_SIZE={os.environ['WORLD_SIZE']}): merging tables of several ranks is not implemented")


def load_run_panel(primers, specimens, sequence_file, args):
    """The panel of a counting run: `args` = a namespace with the matching flags of specimux_amd.cli (-e -E -l --trim
    --dereplicate --disable-prefilter --disable-preorient --min-length --max-length, start_seq / num_seqs); what it lacks
    takes specimux's default.  Returns (namespace, specimens, parameters, prefilter, CompiledPanel)."""
    from . import orchestration
    from .demultiplex import compiled_panel
    ns = argparse.Namespace(primer_file=primers, specimen_file=specimens, sequence_file=sequence_file, index_edit_distance=-1,
                            primer_edit_distance=-1, search_len=80, trim="barcodes", dereplicate="best", disable_prefilter=False,
                            disable_preorient=False, min_length=-1, max_length=-1, start_seq=1, num_seqs=-1, diagnostics=None)
    for k, v in vars(args).items():
        if k in vars(ns) and k not in ("primer_file", "specimen_file", "sequence_file"):
            setattr(ns, k, v)
    specs, parameters, prefilter = orchestration._load(ns)
    return ns, specs, parameters, prefilter, compiled_panel(specs, parameters, ns, prefilter)


def file_batches(reader, panel, ns, batch_reads):
    """The window batches (windows, lens, sequences by index) of the reads ns.start_seq / ns.num_seqs select from `reader`."""
    to_skip, left = max(0, ns.start_seq - 1), (ns.num_seqs if ns.num_seqs >= 0 else None)
    while to_skip > 0:
        b = reader.next_batch(min(to_skip, batch_reads))
        if b is None:
            return
        to_skip -= len(b)
        b.close()
    while left is None or left > 0:
        b = reader.next_batch(batch_reads if left is None else min(batch_reads, left))
        if b is None:
            return
        if left is not None:
            left -= len(b)
        windows, lens = b.pack_windows(panel.search_len, panel.window_stride)
        yield windows, lens, _BatchSeqs(b)


def collect_run_table(primers, specimens, sequence_file, args, capacity=DEFAULT_TABLE_CAPACITY, batch_reads=RUN_BATCH_READS,
                      info=None) -> StatsTable:
    """Demultiplex `sequence_file` on the GPU for counting only and return its stats table.  `args`: as for load_run_panel.
    `info` (dict) receives reads, distinct_keys, host_replayed, counts."""
    refuse_distributed("specimux-stats --from-run")
    import time
    t0 = time.perf_counter()
    from .native_io import Reader
    ns, specs, parameters, prefilter, panel = load_run_panel(primers, specimens, sequence_file, args)
    stats = DeviceStats(panel, capacity)
    replay = HostReplay(panel, parameters, specs, ns, prefilter is not None)
    table = StatsTable()
    reader = Reader(sequence_file)
    t1 = time.perf_counter()
    try:
        counts = accumulate_batches(panel, stats, file_batches(reader, panel, ns, batch_reads), replay, table, n_slots=3,
                                    max_reads=batch_reads)
        keys, cnts = stats.read()
    finally:
        reader.close()
        stats.close()
    table_from_keys(panel, keys, cnts, table)
    if info is not None:
        info.update(reads=int(counts[0]), distinct_keys=len(keys), host_replayed=table.host_replayed, counts=counts,
                    setup_seconds=t1 - t0, count_seconds=time.perf_counter() - t1)
    return table


class _BatchSeqs:
    """Sequences of a native batch by index (only the host-replayed reads are ever asked for)."""

    def __init__(self, batch):
        self.batch = batch

    def __getitem__(self, i):
        return self.batch.record(int(i))[1]


# ------------------------------------------------------------------------------------------------ command line
def build_parser():
    parser = argparse.ArgumentParser(
        prog="specimux-stats", description="Match statistics of a specimux run from its trace events or straight from the GPU",
        formatter_class=argparse.RawDescriptionHelpFormatter,
        epilog="""
Examples:
  %(prog)s trace/ --hierarchical pool primer_pair outcome
  %(prog)s trace/ --hierarchical orientation outcome --count-by sequences
  %(prog)s trace/ --sankey-data pool match_type outcome --output flow.json
  %(prog)s trace/ --list-dimensions
  %(prog)s --from-run primers.fasta specimens.txt reads.fastq --save-table run.json --hierarchical pool outcome
  %(prog)s --table run.json --hierarchical pool primer_pair outcome_detailed
""")
    parser.add_argument("trace_directory", nargs="?", help="Directory containing trace TSV files")
    parser.add_argument("--from-run", nargs=3, metavar=("PRIMERS", "SPECIMENS", "SEQUENCE_FILE"),
                        help="count a run on the GPU (no output tree, no trace) instead of reading a trace directory; takes the "
                             "matching flags of specimux: -e -E -l --trim --dereplicate --disable-prefilter --disable-preorient "
                             "--min-length --max-length -n")
    parser.add_argument("--table", metavar="FILE", help="report from a table written by --save-table instead of a source")
    parser.add_argument("--save-table", metavar="FILE", help="write the stats table (JSON) for later --table queries")
    parser.add_argument("--table-capacity", type=int, default=DEFAULT_TABLE_CAPACITY,
                        help=f"--from-run: slots of the device table (default {DEFAULT_TABLE_CAPACITY}); the run fails if it fills up")
    group = parser.add_mutually_exclusive_group(required=True)
    group.add_argument("--hierarchical", nargs="+", metavar="DIMENSION", help="Generate hierarchical text output with specified dimensions")
    group.add_argument("--sankey-data", nargs="+", metavar="DIMENSION", help="Generate Sankey flow data (JSON) with specified dimensions")
    group.add_argument("--list-dimensions", action="store_true", help="List available dimensions and exit")
    parser.add_argument("--count-by", choices=list(COUNT_MODES), default="candidate_matches",
                        help="Count by candidate matches or unique sequences (default: candidate_matches)")
    parser.add_argument("--output", "-o", help="Output file (default: stdout for hierarchical, required for sankey-data)")
    from . import cli
    run = parser.add_argument_group("--from-run: the matching flags of specimux")
    for flags, kwargs in cli._OPTIONS:
        if _RUN_FLAGS & set(flags):
            run.add_argument(*flags, **kwargs)
    return parser


def main(argv=None):
    """argv without the program name; returns the exit status.  Messages go to stderr as "LEVEL - text", as in the reference."""
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
    args = cli.split_num_seqs(parser, args)
    if sum(x is not None for x in (args.trace_directory, args.from_run, args.table)) != 1:
        parser.error("give exactly one source: trace_directory, --from-run or --table")
    try:
        if args.table:
            table = StatsTable.load(args.table)
        elif args.from_run:
            info = {}
            table = collect_run_table(*args.from_run, args, capacity=args.table_capacity, info=info)
            logger.info(f"Counted {info['reads']:,} reads on the device: {info['distinct_keys']:,} distinct rows, "
                        f"host_replayed {info['host_replayed']} (start-up -- libraries, HIP context, panel -- {info['setup_seconds']:.2f} s, reading and "
                        f"counting {info['count_seconds']:.2f} s)")
        else:
            table = table_from_trace_dir(args.trace_directory)
        if not table.total():
            logger.error("No candidate matches found in trace files")
            return 1
        if args.save_table:
            table.save(args.save_table)
        agg = StatsAggregator(table)
        if args.list_dimensions:
            print("Available dimensions:")
            for dim in agg.available_dimensions:
                print(f"  {dim}")
            return 0
        if args.hierarchical:
            text = format_hierarchical_output(agg.get_hierarchical_stats(args.hierarchical, args.count_by))
            if args.output:
                with open(args.output, "w") as fh:
                    fh.write(text)
                logger.info(f"Hierarchical stats written to {args.output}")
            else:
                print(text)
        else:
            if not args.output:
                logger.error("--output required for --sankey-data")
                return 1
            data = agg.get_sankey_data(args.sankey_data, args.count_by)
            with open(args.output, "w") as fh:
                json.dump(data, fh, indent=2)
            logger.info(f"Sankey data written to {args.output}")
            logger.info(f"Generated {len(data['nodes'])} nodes and {len(data['links'])} links")
    except Exception as e:
        logger.error(f"Error: {e}")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
