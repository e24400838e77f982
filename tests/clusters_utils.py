"""Helpers of the clusters tests (test_clusters_cpu.py, test_clusters_gpu.py, test_pairs_gpu.py): random reads, the
suite's usual mutation model and a synthetic output tree with known clusters."""
import os
import types

from specimux_amd import clusters


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, rate, alphabet="ACGT"):
    """Per base: a substitution, an insertion behind it or a deletion, each with probability rate / 3."""
    out = []
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            out.append(rng.choice(alphabet))
        elif r < 2 * rate / 3:
            out.append(ch + rng.choice(alphabet))
        elif r >= rate:
            out.append(ch)
    return "".join(out)


def fastq_text(rng, name, seqs, qualities=None):
    """FASTQ text of the reads `seqs`, ids <name>_<i>; quality characters random in Phred 10..40, or the one
    character given per read."""
    out = []
    for i, s in enumerate(seqs):
        q = (qualities[i] * len(s)) if qualities else "".join(chr(33 + rng.randrange(10, 41)) for _ in s)
        out.append(f"@{name}_{i} pool=POOL\n{s}\n+\n{q}\n")
    return "".join(out)


def write_tree(rng, root, error=0.02):
    """A specimux output tree of three specimens under root/full/POOL (and side files that are never inputs):
       S_one    40 reads of one 300-nt template
       S_two    28 + 12 reads of two templates, the second a 25 % mutation of the first, shuffled
       S_six    6 unrelated reads
    every read with `error` per-base error.  Returns {specimen: [template index per read]} (S_six: 0..5)."""
    pool = os.path.join(root, "full", "POOL")
    os.makedirs(os.path.join(root, "full", "subsample", "POOL"), exist_ok=True)
    os.makedirs(pool, exist_ok=True)
    t1 = rand_seq(rng, 300)
    t2 = mutate(rng, t1, 0.25)
    labels = {"S_one": [0] * 40, "S_two": [0] * 28 + [1] * 12, "S_six": list(range(6))}
    rng.shuffle(labels["S_two"])
    one = rand_seq(rng, 300)
    reads = {"S_one": [mutate(rng, one, error) for _ in range(40)],
             "S_two": [mutate(rng, (t1, t2)[x], error) for x in labels["S_two"]],
             "S_six": [mutate(rng, rand_seq(rng, 300), error) for _ in range(6)]}
    for name, seqs in reads.items():
        with open(os.path.join(pool, name + ".fastq"), "w") as fh:
            fh.write(fastq_text(rng, name, seqs))
    for side in ("primers.fastq", "S_one.fastq.mined"):
        with open(os.path.join(pool, side), "w") as fh:
            fh.write("@x\nACGT\n+\nIIII\n")
    with open(os.path.join(root, "full", "subsample", "POOL", "S_one.fastq"), "w") as fh:
        fh.write("@x\nACGT\n+\nIIII\n")
    return labels


def run_tool(root, out_dir, adjacency_fn, fastq=None, **options):
    """clusters.run on the tree (or one file of it) with every output switched on; returns {output name: bytes}."""
    os.makedirs(out_dir, exist_ok=True)
    argv = ["--fastq", fastq] if fastq else ["--run-dir", root]
    argv += ["--report", os.path.join(out_dir, "report.tsv"), "--json", os.path.join(out_dir, "report.json"),
             "--centres", os.path.join(out_dir, "centres.fasta"), "--split", os.path.join(out_dir, "split")]
    for key, val in options.items():
        argv += ["--" + key.replace("_", "-"), str(val)]
    args = clusters.build_parser().parse_args(argv)
    assert clusters.run(args, adjacency_fn=adjacency_fn) == 0
    files = {}
    for name in ("report.tsv", "report.json", "centres.fasta"):
        with open(os.path.join(out_dir, name), "rb") as fh:
            files[name] = fh.read()
    for d, _dirs, names in os.walk(os.path.join(out_dir, "split")):
        for name in names:
            with open(os.path.join(d, name), "rb") as fh:
                files[os.path.relpath(os.path.join(d, name), out_dir)] = fh.read()
    return files


def report_rows(tsv_bytes):
    lines = tsv_bytes.decode("latin-1").splitlines()
    assert lines[0].split("\t") == list(clusters.COLUMNS)
    return [types.SimpleNamespace(**dict(zip(clusters.COLUMNS, ln.split("\t")))) for ln in lines[1:]]
