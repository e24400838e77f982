#!/usr/bin/env python3
"""specimine: mine candidate sequences from partial barcode matches for clustering (reference:
src/specimux/specimine.py, entry cli.py:113-116).

For one specimen's `full/` FASTQ, the partial reads of its forward / reverse barcode (`partial/<pool>/...`) are
kept if they align to one of the specimen's full reads with identity >= --min-identity, where identity is
1 - d / len(full) and d is the HW (infix) edit distance of the full read in the partial read, limited to
k = int(len(full) * (1 - min_identity)).  Every distance is computed on the GPU (smx_mine_best_identity, HIP kernel
smx_mine.hip); there is no CPU path.  The output `<fastq>.mined` holds the mined partial records with the title
`{id}_mined_{type}_{best:.2f} {title} mined_{type} identity={best:.2f}`.

    python -m specimux_amd.specimine --index INDEX.txt --fastq full/POOL/SPECIMEN.fastq [--partial-forward]
        [--no-partial-reverse] [--min-identity 0.85] [--debug]
    python -m specimux_amd.specimine --index INDEX.txt --run-dir OUT [--level pool|primer-pair] [...]

`mine_specimens(jobs)` mines many specimens in one set of launches (one job = one CLI run).  `--run-dir` / `mine_run`
mines every specimen file under OUT/full/ in device calls planned under a byte budget (SMX_MINE_BUDGET_BYTES), each
partial file read and uploaded once per call; under torch.distributed.run the specimens are split over the ranks
(one GPU each, LOCAL_RANK) and every rank writes only its own specimens' `.mined` files."""
import argparse
import glob
import logging
import os
import re
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import calls
from .io_utils import SeqRecord, parse_fastq

def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Mine additional candidate sequences from partial matches.")
    parser.add_argument("--index", required=True, help="Path to specimen index file (same as used with specimux)")
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("--fastq", help="Path to full match FASTQ file for a specimen")
    source.add_argument("--run-dir", help="specimux output directory: mine every specimen file under RUN_DIR/full/")
    parser.add_argument("--level", choices=("pool", "primer-pair"), default="pool",
                        help="--run-dir: mine full/<pool>/<S>.fastq (pool) or full/<pool>/<pair>/<S>.fastq (default: pool)")
    parser.add_argument("--partial-forward", action="store_true", default=False,
                        help="Include forward partial matches (default: False)")
    parser.add_argument("--no-partial-reverse", action="store_true", default=False,
                        help="Exclude reverse partial matches (included by default)")
    parser.add_argument("--min-identity", type=float, default=0.85,
                        help="Minimum alignment identity for a match (default: 0.85)")
    parser.add_argument("--debug", action="store_true", help="Enable debug logging")
    return parser


def parse_arguments(argv=None):
    return build_parser().parse_args(argv)


def extract_specimen_id(fastq_path: str) -> str:
    """Specimen id from the FASTQ file name, with or without the legacy `sample_` prefix."""
    filename = os.path.basename(fastq_path)
    match = re.match(r"(?:sample_)?(.+)\.fastq", filename)
    if not match:
        raise ValueError(f"Could not extract specimen ID from filename: {filename}")
    return match.group(1)


def read_index(index_file: str) -> Dict[str, Tuple[str, str]]:
    """specimen id -> (forward, reverse) barcode, upper-cased, from one read of the index: columns SampleID / FwIndex /
    RvIndex by header name (else 0 / 2 / 4), rows too short for them skipped, the first row of a specimen wins."""
    table: Dict[str, Tuple[str, str]] = {}
    with open(index_file, "r") as fh:
        header = next(fh).strip().split("\t")
        sample_idx = header.index("SampleID") if "SampleID" in header else 0
        fwd_idx = header.index("FwIndex") if "FwIndex" in header else 2
        rev_idx = header.index("RvIndex") if "RvIndex" in header else 4
        need = max(sample_idx, fwd_idx, rev_idx)
        for line in fh:
            fields = line.strip().split("\t")
            if len(fields) > need and fields[sample_idx] not in table:
                table[fields[sample_idx]] = (fields[fwd_idx].upper(), fields[rev_idx].upper())
    return table


def _barcodes(table: Dict[str, Tuple[str, str]], specimen_id: str) -> Tuple[Optional[str], Optional[str]]:
    """find_barcodes on read_index's table."""
    if specimen_id in table:
        return table[specimen_id]
    logging.error(f"Could not find specimen {specimen_id} in index file")
    return None, None


def find_barcodes(specimen_id: str, index_file: str) -> Tuple[Optional[str], Optional[str]]:
    """(forward, reverse) barcode of the first index row of the specimen, upper-cased; (None, None) if none."""
    return _barcodes(read_index(index_file), specimen_id)


def detect_input_level(fastq_path: str) -> Tuple[str, str, Optional[str]]:
    """(output_root, pool, primer_pair or None) of full/<pool>/X.fastq (pool level) or full/<pool>/<pair>/X.fastq
    (primer-pair level); the first `full` component of the absolute path counts."""
    parts = os.path.abspath(fastq_path).split(os.sep)
    try:
        full_idx = parts.index("full")
    except ValueError:
        raise ValueError(f"Could not find 'full' directory in path: {fastq_path}")
    output_root = os.sep.join(parts[:full_idx])
    remaining = parts[full_idx + 1:-1]
    if len(remaining) == 1:
        return output_root, remaining[0], None
    if len(remaining) == 2:
        return output_root, remaining[0], remaining[1]
    raise ValueError(f"Unexpected path structure: {fastq_path}")


def _find_partial_files(partial_dir: str, fwd_barcode: str, rev_barcode: str, found: Dict[str, List[str]]) -> None:
    """Append the first existing file per barcode (current name, then the legacy `sample_` name) in one directory."""
    if not os.path.isdir(partial_dir):
        return
    for kind, short, barcode in (("forward", "fwd", fwd_barcode), ("reverse", "rev", rev_barcode)):
        if not barcode:
            continue
        for name in (f"barcode_{short}_{barcode}.fastq", f"sample_barcode_{short}_{barcode}.fastq"):
            path = os.path.join(partial_dir, name)
            if os.path.exists(path):
                found[kind].append(path)
                break


def derive_partial_match_filenames(fastq_path: str, fwd_barcode: str, rev_barcode: str) -> Dict[str, List[str]]:
    """{"forward"|"reverse": [partial files]}: partial/<pool>/<pair>/ at primer-pair level, every directory of
    glob(partial/<pool>/*) (in the order glob returns) at pool level.  Empty lists are dropped."""
    found: Dict[str, List[str]] = {"forward": [], "reverse": []}
    output_root, pool, primer_pair = detect_input_level(fastq_path)
    if primer_pair is not None:
        _find_partial_files(os.path.join(output_root, "partial", pool, primer_pair), fwd_barcode, rev_barcode, found)
    else:
        pool_dir = os.path.join(output_root, "partial", pool)
        if os.path.isdir(pool_dir):
            for pp_dir in glob.glob(os.path.join(pool_dir, "*")):
                if os.path.isdir(pp_dir):
                    _find_partial_files(pp_dir, fwd_barcode, rev_barcode, found)
    if fwd_barcode and not found["forward"]:
        logging.warning(f"No forward partial match files found for barcode: {fwd_barcode}")
    if rev_barcode and not found["reverse"]:
        logging.warning(f"No reverse partial match files found for barcode: {rev_barcode}")
    return {k: v for k, v in found.items() if v}


def calculate_identity(alignment_result: Dict, query_length: int) -> float:
    """1 - editDistance / query_length; 0 for a failed alignment (editDistance -1)."""
    d = alignment_result["editDistance"]
    if d == -1:
        return 0
    return 1 - (d / query_length)


def max_distance(full_length: int, min_identity: float) -> int:
    """The edlib limit k of one full read (negative: no limit)."""
    return int(full_length * (1 - min_identity))


def mined_title(record: SeqRecord, partial_type: str, best_identity: float) -> str:
    """Title line (without '@') of a mined record: the id and description the reference sets, joined the way
    Biopython's FASTQ writer joins an id and a description that no longer starts with it."""
    return (f"{record.id}_mined_{partial_type}_{best_identity:.2f} "
            f"{record.description} mined_{partial_type} identity={best_identity:.2f}")


def format_record(title: str, record: SeqRecord) -> str:
    return f"@{title}\n{record.seq}\n+\n{record.quality_string}\n"


def read_fastq(path: str) -> List[SeqRecord]:
    with open(path, "r", encoding="latin-1") as fh:   # one character per byte: the kernel compares bytes
        return list(parse_fastq(fh))


class MineJob:
    """One specimen: its full file, the selected partial files per type and the identity threshold."""

    def __init__(self, fastq: str, partial_files: Dict[str, List[str]], min_identity: float):
        self.fastq = fastq
        self.partial_files = partial_files
        self.min_identity = min_identity
        self.output = f"{fastq}.mined"


def plan_job(index: str, fastq: str, partial_forward: bool = False, no_partial_reverse: bool = False,
             min_identity: float = 0.85) -> MineJob:
    """Everything main() does before mining; exits with status 1 where the reference does."""
    job = _plan(lambda sid: find_barcodes(sid, index), fastq, partial_forward, no_partial_reverse, min_identity)
    if job is None:
        sys.exit(1)
    return job


def _plan(lookup, fastq, partial_forward, no_partial_reverse, min_identity) -> Optional[MineJob]:
    """plan_job with the barcode lookup given; None (the messages logged) where the single CLI exits with status 1."""
    specimen_id = extract_specimen_id(fastq)
    logging.info(f"Processing specimen: {specimen_id}")
    fwd_barcode, rev_barcode = lookup(specimen_id)
    if not (fwd_barcode and rev_barcode):
        return None
    logging.info(f"Found barcodes - Forward: {fwd_barcode}, Reverse: {rev_barcode}")
    partial_files = derive_partial_match_filenames(fastq, fwd_barcode, rev_barcode)
    for ptype, files in partial_files.items():
        logging.info(f"Found {len(files)} {ptype} partial match file(s)")
        for f in files:
            logging.debug(f"  - {f}")
    if not partial_forward and "forward" in partial_files:
        del partial_files["forward"]
    if no_partial_reverse and "reverse" in partial_files:
        del partial_files["reverse"]
    if not partial_files:
        logging.error("No partial match files found or selected")
        return None
    return MineJob(fastq, partial_files, min_identity)


_best_identity = calls.mine_best_identity


def _mine(jobs: Sequence[MineJob], kernel_ms=None):
    """Mine every job in one device call.  Yields per job its mined (title, record) pairs in the reference's order
    (types in dict order, files in discovery order, records in file order), or None for a job whose full file holds
    no records; logs each job as the single CLI does.

    Every partial file is read and uploaded once, however many jobs select it; a device job is one specimen's full
    reads x one partial file (the best identity of a partial read depends only on the specimen's full reads), the
    forward and reverse jobs of a specimen share its query range."""
    files: Dict[str, int] = {}                     # partial file -> index in `parts`
    parts: List[List[SeqRecord]] = []
    fulls_of, queries, ks, targets, djobs = [], [], [], [], []
    t_at: List[int] = []                           # first target of each partial file
    for job in jobs:
        fulls = read_fastq(job.fastq)
        fulls_of.append(fulls)
        if not fulls:
            continue
        q0 = len(queries)
        for r in fulls:
            queries.append(r.seq.encode("latin-1"))
            ks.append(max_distance(len(queries[-1]), job.min_identity))
        for flist in job.partial_files.values():
            for f in flist:
                if f not in files:
                    files[f] = len(parts)
                    parts.append(read_fastq(f))
                    t_at.append(len(targets))
                    targets.extend(r.seq.encode("latin-1") for r in parts[-1])
                i = files[f]
                djobs.append((q0, len(fulls), t_at[i], len(parts[i]), job.min_identity))
    best = _best_identity(queries, ks, targets, djobs, kernel_ms) if djobs else np.zeros(0, dtype=np.float64)
    at = 0                                         # next job's first output
    for job, fulls in zip(jobs, fulls_of):
        if not fulls:
            logging.error(f"No sequences found in full match file: {job.fastq}")
            yield None
            continue
        logging.info(f"Loaded {len(fulls)} sequences from full match file")
        mined = []
        for ptype, flist in job.partial_files.items():
            logging.info(f"Processing {ptype} partial matches from {len(flist)} file(s)")
            n_total = sum(len(parts[files[f]]) for f in flist)
            logging.info(f"Found {n_total} sequences across all {ptype} partial match files")
            match_count = 0
            for f in flist:
                recs = parts[files[f]]
                for rec, b in zip(recs, best[at:at + len(recs)]):
                    if b > 0:
                        match_count += 1
                        mined.append((mined_title(rec, ptype, float(b)), rec))
                at += len(recs)
            logging.info(f"Matched {match_count}/{n_total} sequences from {ptype} partial matches")
        yield mined


def _mine_call(jobs: Sequence[MineJob], kernel_ms=None) -> List[Optional[int]]:
    """Mine every job in one device call (_mine) and write each job's `<fastq>.mined`.  Returns the mined count per
    job, None for a job whose full file holds no records (it gets the empty `.mined` the single CLI writes)."""
    counts: List[Optional[int]] = []
    for job, mined in zip(jobs, _mine(jobs, kernel_ms)):
        out = [format_record(title, rec) for title, rec in mined or []]
        logging.info(f"Found {len(out)} mined sequences")
        with open(job.output, "w", encoding="latin-1") as fh:
            fh.write("".join(out))
        logging.info(f"Wrote {len(out)} sequences to {job.output}")
        counts.append(None if mined is None else len(out))
    return counts


def mine_specimens(jobs: Sequence[MineJob], kernel_ms=None) -> List[int]:
    """Mine every job in one device call and write each job's `<fastq>.mined`; returns the mined count per job."""
    return [c or 0 for c in _mine_call(jobs, kernel_ms)]


# ------------------------------------------------------------------------------------------------ whole-run mining
DEFAULT_BUDGET_BYTES = 1 << 30   # FASTQ bytes (full + distinct partial files) per device call


def discover_specimens(output_dir: str, level: str = "pool") -> List[str]:
    """The specimen files of a specimux output tree, sorted: full/<pool>/<S>.fastq (level "pool") or
    full/<pool>/<pair>/<S>.fastq (level "primer-pair").  `.mined` files, `primers.*` and `subsample/` are never inputs."""
    if level not in ("pool", "primer-pair"):
        raise ValueError(f"unknown level: {level}")
    full = os.path.join(output_dir, "full")
    dirs = []
    if os.path.isdir(full):
        for pool in sorted(os.listdir(full)):
            pool_dir = os.path.join(full, pool)
            if pool == "subsample" or not os.path.isdir(pool_dir):
                continue
            if level == "pool":
                dirs.append(pool_dir)
            else:
                dirs.extend(os.path.join(pool_dir, pair) for pair in sorted(os.listdir(pool_dir))
                            if pair != "subsample" and os.path.isdir(os.path.join(pool_dir, pair)))
    out = []
    for d in dirs:
        for name in sorted(os.listdir(d)):
            path = os.path.join(d, name)
            if name.endswith(".fastq") and not name.startswith("primers.") and os.path.isfile(path):
                out.append(path)
    return out


def job_partials(job: MineJob) -> List[str]:
    """The partial files a job reads, each once, in job order."""
    return list(dict.fromkeys(f for flist in job.partial_files.values() for f in flist))


def plan_shards(items: Sequence[Tuple[int, Sequence[str]]], world: int) -> List[List[int]]:
    """Split specimens over `world` ranks.  items[i] = (work of specimen i, its partial files).  Specimens that share a
    partial file form a group.  Units (whole groups, or single specimens) go largest first, ties by first specimen,
    each to the rank with the least work so far (ties: the lowest rank).  Groups up to total / world, then up to
    total / (2 * world) stay whole; the first of these splits whose busiest rank is within the bound is taken, else
    every specimen is a unit of its own (which always is).  Deterministic; every rank's work is at most
    total / world + the largest specimen's work.  Returns the sorted specimen indices per rank."""
    n = len(items)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    owner: Dict[str, int] = {}
    for i, (_, pfiles) in enumerate(items):
        for f in pfiles:
            if f in owner:
                a, b = find(i), find(owner[f])
                if a != b:
                    parent[max(a, b)] = min(a, b)
            else:
                owner[f] = i
    groups: Dict[int, List[int]] = {}
    for i in range(n):
        groups.setdefault(find(i), []).append(i)
    total = sum(w for w, _ in items)
    bound = total / world + max((w for w, _ in items), default=0)

    def assign(limit):
        units = []
        for members in groups.values():
            work = sum(items[i][0] for i in members)
            if work <= limit or len(members) == 1:
                units.append((work, members))
            else:
                units.extend((items[i][0], [i]) for i in members)
        units.sort(key=lambda u: (-u[0], u[1][0]))
        load = [0] * world
        shards: List[List[int]] = [[] for _ in range(world)]
        for work, members in units:
            r = min(range(world), key=lambda x: (load[x], x))
            load[r] += work
            shards[r].extend(members)
        return max(load), [sorted(s) for s in shards]

    for limit in (total / world, total / (2 * world)):
        busiest, shards = assign(limit)
        if busiest <= bound:
            return shards
    return assign(-1)[1]


def plan_calls(items: Sequence[Tuple[int, Sequence[Tuple[str, int]]]], budget: int) -> List[List[int]]:
    """Group specimens into device calls.  items[i] = (bytes of specimen i's full file, [(partial file, bytes)]).  A
    call costs its full files plus its distinct partial files; specimens that share partial files are taken one
    after the other (ordered by their first partial file) so that they land in the same call, and a call is closed
    before it would exceed `budget`.  A specimen that alone exceeds the budget gets a call of its own."""
    order = sorted(range(len(items)), key=lambda i: (min((f for f, _ in items[i][1]), default=""), i))
    calls: List[List[int]] = []
    cur: List[int] = []
    seen: set = set()
    cost = 0
    for i in order:
        full_bytes, pfiles = items[i]
        extra = full_bytes + sum(b for f, b in pfiles if f not in seen)
        if cur and cost + extra > budget:
            calls.append(cur)
            cur, seen, cost = [], set(), 0
            extra = full_bytes + sum(b for _, b in pfiles)
        cur.append(i)
        seen.update(f for f, _ in pfiles)
        cost += extra
    if cur:
        calls.append(cur)
    return calls


def call_cost(items, call) -> int:
    """Bytes a call of plan_calls reads: its full files and its distinct partial files."""
    pfiles = {f: b for i in call for f, b in items[i][1]}
    return sum(items[i][0] for i in call) + sum(pfiles.values())


def budget_bytes() -> int:
    env = os.environ.get("SMX_MINE_BUDGET_BYTES")
    return int(env) if env else DEFAULT_BUDGET_BYTES


def mine_run(output_dir: str, index: str, level: str = "pool", partial_forward: bool = False,
             no_partial_reverse: bool = False, min_identity: float = 0.85, rank: int = 0, world: int = 1,
             budget: Optional[int] = None, kernel_ms=None) -> Dict[str, int]:
    """Mine every specimen file under output_dir/full/ (discover_specimens) that rank `rank` of `world` owns
    (plan_shards) and write each one's `.mined`, byte-identical to one single-file CLI run per specimen.  A specimen
    the single CLI would refuse (no index row, no partial file selected) is logged the same way and skipped; a full
    file without records is logged as there and gets the same empty `.mined`, and counts as skipped.  Returns
    {"specimens", "planned", "mined", "skipped", "reads"}: specimens / planned over the whole run, the rest over
    this rank's specimens plus (every rank) the specimens that could not be planned."""
    fastqs = discover_specimens(output_dir, level)
    table = read_index(index)
    quiet = rank != 0                              # every rank plans the whole run; rank 0 logs it
    if quiet:
        logging.disable(logging.CRITICAL)
    try:
        planned = [_plan(lambda sid: _barcodes(table, sid), f, partial_forward, no_partial_reverse, min_identity)
                   for f in fastqs]
    finally:
        if quiet:
            logging.disable(logging.NOTSET)
    jobs = [j for j in planned if j is not None]
    result = {"specimens": len(fastqs), "planned": len(jobs), "mined": 0,
              "skipped": len(fastqs) - len(jobs), "reads": 0}
    if not jobs:
        return result
    size = os.path.getsize
    sizes = [(size(j.fastq), [(f, size(f)) for f in job_partials(j)]) for j in jobs]
    mine = plan_shards([(fb * sum(b for _, b in pf), [f for f, _ in pf]) for fb, pf in sizes], world)[rank]
    mine_items = [sizes[i] for i in mine]
    for call in plan_calls(mine_items, budget if budget is not None else budget_bytes()):
        for c in _mine_call([jobs[mine[i]] for i in call], kernel_ms):
            if c is None:
                result["skipped"] += 1
            else:
                result["mined"] += 1
                result["reads"] += c
    return result


def _summary(res: Dict[str, int]) -> str:
    return (f"Mined {res['mined']} specimen(s), skipped {res['skipped']} of {res['specimens']}; "
            f"{res['reads']} mined sequences in total")


def run_main(args) -> int:
    """--run-dir: this process's share of the run (torch.distributed.run: RANK / LOCAL_RANK / WORLD_SIZE, one GPU per
    rank, gloo for the summary).  Returns the exit status: 1 if no specimen could be planned."""
    from . import _lib
    from .distributed import env_rank
    rank, local_rank, world = env_rank()
    n_dev = _lib.C.c_int(0)
    lib = _lib.load()
    _lib.check(lib.smx_device_init(0, _lib.C.byref(n_dev)))
    _lib.check(lib.smx_device_init(local_rank % n_dev.value, None))   # more ranks than GPUs: ranks share them
    kw = dict(level=args.level, partial_forward=args.partial_forward, no_partial_reverse=args.no_partial_reverse,
              min_identity=args.min_identity)
    if world == 1:
        res = mine_run(args.run_dir, args.index, rank=0, world=1, **kw)
    else:
        import torch
        import torch.distributed as dist
        own_group = not dist.is_initialized()
        if own_group:
            dist.init_process_group("gloo")
        try:
            err, res = None, None
            try:
                res = mine_run(args.run_dir, args.index, rank=rank, world=world, **kw)
            except Exception as e:   # noqa: BLE001 -- re-raised after the ranks agree, so that none waits in a collective
                err = e
            # mined specimens and reads are per rank; specimens, planned and the planning skips are the same on every rank
            mine = res or {"specimens": 0, "planned": 0, "mined": 0, "skipped": 0, "reads": 0}
            unplanned = mine["specimens"] - mine["planned"]
            t = torch.tensor([err is not None, mine["mined"], mine["skipped"] - unplanned, mine["reads"]], dtype=torch.int64)
            dist.all_reduce(t)                     # also the barrier before rank 0's summary
            if err is not None:
                raise err
            if int(t[0]):
                raise RuntimeError("specimine: another rank failed")
            res = dict(mine, mined=int(t[1]), skipped=int(t[2]) + unplanned, reads=int(t[3]))
        finally:
            if own_group:
                dist.destroy_process_group()
    if res["planned"] == 0:
        if rank == 0:
            logging.error("No specimen could be planned")
        return 1
    if rank == 0:
        logging.info(_summary(res))
    return 0


def mine_sequences(full_match_file: str, partial_match_files: Dict[str, List[str]],
                   min_identity: float) -> List[Tuple[str, SeqRecord]]:
    """The mined records of one specimen as (title, record) pairs, in the reference's order (types in dict order,
    files in discovery order, records in file order)."""
    return next(_mine([MineJob(full_match_file, partial_match_files, min_identity)])) or []


# ------------------------------------------------------------------------------------------------ shared by the tools
def permille(share: float) -> int:
    return int(round(share * 1000))


def write_texts(pairs) -> None:
    """Write each (path, function that returns the text) whose path is set, one character per byte."""
    for dest, text in pairs:
        if dest:
            with open(dest, "w", encoding="latin-1") as fh:
                fh.write(text())


def tool_main(build_parser, run, argv=None, value_error_status=None) -> None:
    """The main() the tools share: parse, set the logging up, run(args) and exit with its status if that is not 0.  With
    value_error_status a ValueError out of run() is logged and becomes that status."""
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if args.debug else logging.INFO,
                        format="%(asctime)s - %(levelname)s - %(message)s")
    try:
        status = run(args)
    except ValueError as e:
        if value_error_status is None:
            raise
        logging.error(str(e))
        status = value_error_status
    if status:
        sys.exit(status)


def main(argv=None):
    args = parse_arguments(argv)
    logging.basicConfig(level=logging.DEBUG if args.debug else logging.INFO,
                        format="%(asctime)s - %(levelname)s - %(message)s")
    if args.run_dir is not None:
        status = run_main(args)
        if status:
            sys.exit(status)
        return
    job = plan_job(args.index, args.fastq, args.partial_forward, args.no_partial_reverse, args.min_identity)
    mine_specimens([job])


if __name__ == "__main__":
    main()
