"""A synthetic demultiplexed run for the crosstalk tests: six specimens of one pool, built from random 300-nt templates
with reads at 3 % error and fixed seeds, each planted with one of the outcomes specimux-crosstalk tells apart.

    A   20 reads of its own template and 6 reads of B's: a leak, A <- B flagged with 6 reads
    B   20 reads of its own
    C   20 reads of its own and 3 reads of D's template; D's template is C's with 3 substitutions, so those reads are
        nearer to D's ref but `ambiguous` (the refs are fewer than --min-separation apart), never foreign, never flagged
    D   20 reads of its own
    E   an empty well: only 5 reads of B's template, and no ref: `no_reference`, all foreign, E <- B flagged with 5 reads
    F   20 reads of its own and 4 junk reads: `unplaced`

The refs are the templates themselves, `<specimen>_c1`, plus `GHOST_c1`, a random sequence that matches no file."""
import json
import os
import random
from types import SimpleNamespace

SPECIMENS = ("SPEC_A", "SPEC_B", "SPEC_C", "SPEC_D", "SPEC_E", "SPEC_F")
LENGTH, ERROR = 300, 0.03


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(rng, s, rate):
    out = []
    for c in s:
        r = rng.random()
        if r < rate / 3:
            out.append(rng.choice("ACGT".replace(c, "")))
        elif r < 2 * rate / 3:
            out.append(c + rng.choice("ACGT"))
        elif r >= rate:
            out.append(c)
    return "".join(out)


def templates(seed=11):
    rng = random.Random(seed)
    t = {s: rand_seq(rng, LENGTH) for s in ("SPEC_A", "SPEC_B", "SPEC_C", "SPEC_F", "GHOST")}
    d = list(t["SPEC_C"])
    for p in (40, 150, 260):                       # three substitutions: NW distance 3
        d[p] = "ACGT"[("ACGT".index(d[p]) + 1) % 4]
    t["SPEC_D"] = "".join(d)
    return t


def build_run(root, seed=11, pool="pool1"):
    """Writes root/full/<pool>/<S>.fastq for the six specimens, root/refs.fasta and root/consensus.json (the refs in the
    shape of specimux-consensus --json).  Returns {specimen: path}."""
    rng = random.Random(seed * 7919 + 1)
    t = templates(seed)
    plan = {"SPEC_A": [("SPEC_A", 20), ("SPEC_B", 6)], "SPEC_B": [("SPEC_B", 20)], "SPEC_C": [("SPEC_C", 20), ("SPEC_D", 3)],
            "SPEC_D": [("SPEC_D", 20)], "SPEC_E": [("SPEC_B", 5)], "SPEC_F": [("SPEC_F", 20), (None, 4)]}
    d = os.path.join(root, "full", pool)
    os.makedirs(d, exist_ok=True)
    paths = {}
    for spec in SPECIMENS:
        reads = []
        for src, n in plan[spec]:
            for _ in range(n):
                reads.append(mutate(rng, t[src], ERROR) if src else rand_seq(rng, LENGTH))
        rng.shuffle(reads)
        paths[spec] = os.path.join(d, spec + ".fastq")
        with open(paths[spec], "w") as fh:
            for i, s in enumerate(reads):
                q = "".join(chr(33 + rng.randint(8, 40)) for _ in s)
                fh.write(f"@{spec}_r{i} extra words\n{s}\n+\n{q}\n")
    with_ref = ("SPEC_A", "SPEC_B", "SPEC_C", "SPEC_D", "SPEC_F")
    with open(os.path.join(root, "refs.fasta"), "w") as fh:
        for spec in with_ref + ("GHOST",):
            fh.write(f">{spec}_c1 size=20 share=1.0000\n{t[spec][:150]}\n{t[spec][150:]}\n")
    doc = {"summary": {}, "specimens": [{"specimen": paths[s], "clusters": [{"name": s + "_c1", "rank": 1, "consensus": t[s]}]}
                                        for s in with_ref]}
    doc["specimens"].append({"specimen": os.path.join(d, "GHOST.fastq"), "clusters": [{"name": "GHOST_c1", "rank": 1, "consensus": t["GHOST"]}]})
    with open(os.path.join(root, "consensus.json"), "w") as fh:
        json.dump(doc, fh)
    return paths


def args_for(root, out, **kw):
    """The parsed arguments of one tool run that writes out/report.tsv, out/report.json and out/reads.tsv."""
    os.makedirs(out, exist_ok=True)
    a = dict(run_dir=os.fspath(root), level="pool", consensus=None, refs=os.path.join(root, "refs.fasta"), min_identity=0.90,
             max_reads=0, min_separation=5, min_reads=5, report=os.path.join(out, "report.tsv"),
             json=os.path.join(out, "report.json"), reads=os.path.join(out, "reads.tsv"), debug=False)
    a.update(kw)
    return SimpleNamespace(**a)


def outputs(out):
    return {name: open(os.path.join(out, name), "rb").read() for name in ("report.tsv", "report.json", "reads.tsv")}
