"""A synthetic reference database for the identify tests: about 200 unrelated refs of 400-500 nt with fixed seeds, and
eight queries, each planted with one of the outcomes specimux-identify tells apart (--min-identity 0.90, --top 5).

    Q_FLANK   its ref REF_FLANK carries 60-nt flanks the query lacks: the query is the pattern; unique
    Q_TRIM    its ref REF_TRIM is trimmed, the query carries 60-nt flanks: the ref is the pattern; unique
    Q_RC      its ref REF_RC is in the database only reverse-complemented: a `-` hit with --strand both, none with plus
    Q_TIED    two identical refs under the names TWIN_A and TWIN_B: tied
    Q_SAME    two identical refs under the one name SAME_NAME: unique
    Q_LIMIT   LIMIT_IN is the query with exactly k substitutions, LIMIT_OUT with k + 1 (k = the query's limit): only
              LIMIT_IN is a hit
    Q_FRAG    FRAG is a 120-nt piece of the 400-nt query: --min-coverage 0.5 excludes it (none), 0.1 admits it
    Q_NONE    a random sequence: none

The database file is written wrapped at 70 columns, every third record in lower case."""
import gzip
import os
import random
from types import SimpleNamespace

from specimux_amd import identify, specimine

MIN_IDENTITY = 0.90
QUERIES = ("Q_FLANK", "Q_TRIM", "Q_RC", "Q_TIED", "Q_SAME", "Q_LIMIT", "Q_FRAG", "Q_NONE")


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def substitute(rng, s, n):
    """s with exactly n substitutions at positions a fixed stride apart."""
    out = list(s)
    stride = len(s) // (n + 1)
    for i in range(n):
        p = stride * (i + 1)
        out[p] = rng.choice("ACGT".replace(out[p], ""))
    return "".join(out)


def build(seed=23, n_background=190):
    """(queries, refs): lists of (header line, sequence)."""
    rng = random.Random(seed)
    q = {"Q_FLANK": rand_seq(rng, 300), "Q_RC": rand_seq(rng, 320), "Q_TIED": rand_seq(rng, 310), "Q_SAME": rand_seq(rng, 305),
         "Q_LIMIT": rand_seq(rng, 300), "Q_FRAG": rand_seq(rng, 400), "Q_NONE": rand_seq(rng, 330)}
    core = rand_seq(rng, 300)
    q["Q_TRIM"] = rand_seq(rng, 60) + core + rand_seq(rng, 60)
    k = specimine.max_distance(len(q["Q_LIMIT"]), MIN_IDENTITY)
    planted = [
        ("REF_FLANK Fungus flankii voucher 1", rand_seq(rng, 60) + substitute(rng, q["Q_FLANK"], 2) + rand_seq(rng, 60)),
        ("REF_TRIM Fungus trimmii", substitute(rng, core, 3)),
        ("REF_RC Fungus reversus", identify.revcomp(substitute(rng, q["Q_RC"], 1).encode()).decode()),
        ("TWIN_A Fungus geminus strain A", rand_seq(rng, 10) + q["Q_TIED"] + rand_seq(rng, 10)),
        ("SAME_NAME copy 1", "G" + q["Q_SAME"] + "T"),
        ("LIMIT_IN inside the limit", rand_seq(rng, 20) + substitute(rng, q["Q_LIMIT"], k) + rand_seq(rng, 20)),
        ("LIMIT_OUT outside the limit", rand_seq(rng, 20) + substitute(rng, q["Q_LIMIT"], k + 1) + rand_seq(rng, 20)),
        ("FRAG a fragment", q["Q_FRAG"][100:220]),
    ]
    planted.append(("TWIN_B Fungus geminus strain B", planted[3][1]))
    planted.append(("SAME_NAME copy 2", planted[4][1]))
    refs = [(f"BG{i:03d} background {i}", rand_seq(rng, rng.randrange(400, 501))) for i in range(n_background)]
    for i, rec in enumerate(planted):              # spread over the file, so that pieces of the database split them up
        refs.insert((i * 19 + 7) % len(refs), rec)
    return [(name, q[name]) for name in QUERIES], refs


def write_fasta(path, records, wrap=70, lower_every=0, gz=False):
    lines = []
    for i, (title, seq) in enumerate(records):
        if lower_every and i % lower_every == 0:
            seq = seq.lower()
        lines.append(">" + title)
        lines += [seq[a:a + wrap] for a in range(0, len(seq), wrap)] if wrap else [seq]
    text = "\n".join(lines) + "\n"
    with (gzip.open(path, "wt", encoding="latin-1") if gz else open(path, "w", encoding="latin-1")) as fh:
        fh.write(text)


def build_files(root):
    """Writes root/queries.fasta, root/db.fasta (wrapped, partly lower case), root/db.fasta.gz and root/db_plain.fasta (one
    line per record, upper case).  Returns (queries, refs)."""
    queries, refs = build()
    write_fasta(os.path.join(root, "queries.fasta"), queries, wrap=0)
    write_fasta(os.path.join(root, "db.fasta"), refs, wrap=70, lower_every=3)
    write_fasta(os.path.join(root, "db.fasta.gz"), refs, wrap=70, lower_every=3, gz=True)
    write_fasta(os.path.join(root, "db_plain.fasta"), refs, wrap=0)
    return queries, refs


def args_for(root, out_dir, db="db.fasta", **kw):
    os.makedirs(out_dir, exist_ok=True)
    base = dict(consensus=None, fasta=os.path.join(root, "queries.fasta"), db=os.path.join(root, db), min_identity=MIN_IDENTITY,
                top=5, min_coverage=0.5, strand="both", report=os.path.join(out_dir, "report.tsv"),
                json=os.path.join(out_dir, "report.json"), debug=False)
    base.update(kw)
    return SimpleNamespace(**base)


def outputs(out_dir):
    out = {}
    for name in ("report.tsv", "report.json"):
        with open(os.path.join(out_dir, name), "r", encoding="latin-1") as fh:
            out[name] = fh.read()
    return out


def rows_of(tsv):
    """{query: [row dict, ...]} of a --report file."""
    lines = tsv.rstrip("\n").split("\n")
    assert tuple(lines[0].split("\t")) == identify.COLUMNS
    out = {}
    for line in lines[1:]:
        row = dict(zip(identify.COLUMNS, line.split("\t")))
        out.setdefault(row["query"], []).append(row)
    return out


def three_piece_budget(queries, refs, strands=2):
    """A budget under which the database falls into three pieces."""
    return sum(len(s) for _, s in queries) + strands * sum(len(s) for _, s in refs) // 3 + 600
