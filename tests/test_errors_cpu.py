"""specimux-errors without a GPU: the percentile and binomial arithmetic on hand-computed cases, the twin's invariants on
random input, the argument errors, and the tool end to end over a small synthetic plate with the plain-Python twins of
its device calls (clusters.adjacency_oracle, cons_utils.votes_reference, variants_utils.phase_reference,
errors_utils.profile_reference)."""
import json
import os
import random
import types

import numpy as np
import pytest

from clusters_utils import mutate, rand_seq
from cons_utils import row_reference, votes_reference
from errors_utils import HP, INS, Q, SUBST, draft_runs, member_profile, profile_reference
from specimux_amd import clusters, errors
from test_variants_cpu import write_specimen
from variants_utils import phase_reference

OUTPUTS = ("errors.tsv", "quality.tsv", "homopolymers.tsv", "reads.tsv", "errors.json", "called.fasta")
TWINS = dict(adjacency_fn=clusters.adjacency_oracle, votes_fn=votes_reference, phase_fn=phase_reference)
SUBS_PER_READ = 3


# ------------------------------------------------------------------------------------------------ the arithmetic
def test_percentiles_are_nearest_rank():
    assert [errors.percentile_rank(p, 20) for p in (5, 50, 95)] == [0, 9, 18]
    assert [errors.percentile_rank(p, 100) for p in (5, 50, 95)] == [4, 49, 94]
    assert [errors.percentile_rank(p, 1) for p in (5, 50, 95)] == [0, 0, 0]
    assert [errors.percentile_rank(p, 21) for p in (5, 50, 95)] == [1, 10, 19]       # ceil(1.05), ceil(10.5), ceil(19.95)
    # ordered by the exact fraction, not by a float: 1/3 < 333334/1000000 < 2/3
    parts = [(2, 3), (333334, 1000000), (1, 3)] + [(9, 10)] * 17
    assert errors.identity_percentiles(parts) == [(1, 3), (9, 10), (9, 10)]
    assert errors.identity_percentiles([]) == [None, None, None]
    assert errors.identity_parts([90, 3, 2, 1, 2, 4, 0, 0]) == (90, 100)
    assert errors.fmt_identity((90, 100)) == "0.9000" and errors.fmt_identity(None) == "-" and errors.fmt_rate(3, 2000) == "1.500"


def test_binomial_shares():
    assert errors.more_than(1, 0, 1, 10) == pytest.approx(0.1)
    assert errors.more_than(2, 0, 1, 2) == pytest.approx(0.75) and errors.more_than(2, 1, 1, 2) == pytest.approx(0.25)
    assert errors.more_than(2, 2, 1, 2) == 0.0 and errors.more_than(2, 4, 1, 2) == 0.0
    assert errors.more_than(13, 0, 0, 100) == 0.0 and errors.more_than(13, 0, 5, 0) == 0.0
    assert errors.more_than(3, 0, 7, 5) == 1.0                 # a rate above 1 counts as 1
    # 20 bases at 5 %: P(X > 1) = 1 - 0.95^20 - 20 * 0.05 * 0.95^19
    assert errors.more_than(20, 1, 5, 100) == pytest.approx(1 - 0.95**20 - 20 * 0.05 * 0.95**19)
    assert errors.parse_lengths("20, 13,13") == [13, 20]
    assert errors.predicted_error_permille("+5I") == pytest.approx(1000 * (0.1 + 0.01 + 0.0001) / 3)
    assert errors.predicted_error_permille("") is None


def test_totals_count_the_members_that_did_not_align():
    tables = np.zeros(274, dtype=np.uint32)
    tables[HP + 2 * 7 + 3], tables[HP + 2 * 7 + 2], tables[HP + 7 * 7 + 6], tables[HP + 3] = 6, 1, 1, 50
    members = np.array([[8, 1, 1, 0, 1, 2, 0, 0], [0] * 8, [10, 0, 0, 0, 1, 255, 1, 0]], dtype=np.uint32)
    t = errors.Totals("S")
    t.add_job(errors.JobProfile(None, 2, members, tables))
    assert (t.members, t.aligned, t.not_aligned, t.clipped, t.bases, t.errors) == (3, 2, 1, 1, 20, 1 + 1 + 257)
    assert t.parts == [(8, 12), (10, 265)] and t.hp_long() == (2, 8)
    row = dict(zip(errors.COLUMNS, errors.report_row(t)))
    assert row["not_aligned"] == "1" and row["sub_per_kb"] == "50.000" and row["hp_off"] == "0.2500" and row["identity_p50"] == "0.0377"


# ------------------------------------------------------------------------------------------------ the twin's invariants
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_twin_invariants_on_random_input(seed):
    """Over members with substitutions, indels and `N` bytes around a draft of bases with runs: the sum of c_p is the read's
    length; every row of hp sums to (the draft's runs of that class) x aligned; subst and other together hold every column
    of every aligned member once."""
    rng = random.Random(seed)
    draft = "".join(rng.choice("ACGT") * rng.choice([1, 1, 2, 3, 5, 9]) for _ in range(40))
    m = len(draft)
    reads = [mutate(rng, draft, 0.08, "ACGTN") for _ in range(25)] + [rand_seq(rng, m)] + [draft]
    raw = [r.encode() for r in reads]
    quals = [bytes(rng.randrange(33, 127) for _ in r) for r in reads]
    ks = [m // 4] * len(reads)
    (table, aligned, words, tables), = profile_reference(raw, quals, ks, [(26, 0, 26)])
    assert aligned == 25 and not words[25].any()               # the unrelated read is above its limit
    for i in range(25):
        d, row = row_reference(raw[26], raw[i], m // 4)
        w, _t, consumed = member_profile(raw[26], row, quals[i])
        assert consumed == len(reads[i]) and w[0] + w[1] + w[2] + w[3] == m and w[:6] == words[i, :6].tolist()
        assert w[0] + w[1] + w[3] + w[5] == len(reads[i])      # the read's bases: its columns' and its inserted ones
    classes = [0] * 8
    for _s, r, _b in draft_runs(raw[26]):
        classes[min(r, 8) - 1] += 1
    assert tables[HP:].reshape(8, 7).sum(axis=1).tolist() == [c * aligned for c in classes] and classes[7] > 0
    assert int(tables[SUBST:SUBST + 20].sum()) + int(words[:, 3].sum()) == aligned * m
    assert int(tables[Q:Q + 192].sum()) == sum(len(reads[i]) for i in range(25))
    assert int(tables[INS:INS + 6].sum()) == int(words[:, 5].sum()) and words[:, 3].sum() > 0


# ------------------------------------------------------------------------------------------------ the tool
def homopolymer_template(rng, n=300):
    t = list(rand_seq(rng, n))
    t[99], t[100:108], t[108] = "C", "A" * 8, "G"
    return "".join(t)


@pytest.fixture(scope="module")
def plate(tmp_path_factory):
    """Three specimens under root/full/POOL, 30 reads of a 300-nt template with an 8-base homopolymer each:
       S_noisy   at 5 % error, ten of the reads with the homopolymer a base short
       S_clean   at 1 %
       S_subs    exact copies but for SUBS_PER_READ substitutions per read, at columns no two reads share"""
    root = str(tmp_path_factory.mktemp("plate"))
    rng = random.Random(131)
    noisy, clean, subs = (homopolymer_template(rng) for _ in range(3))
    write_specimen(root, "S_noisy", rng, [mutate(rng, noisy[:100] + noisy[101:] if i % 3 == 0 else noisy, 0.05) for i in range(30)])
    write_specimen(root, "S_clean", rng, [mutate(rng, clean, 0.01) for _ in range(30)])
    reads = []
    for i in range(30):
        r = list(subs)
        for x in range(SUBS_PER_READ):
            p = 5 + i * 3 + x * 97                             # 5..286: distinct over reads and x
            r[p] = "ACGT"[("ACGT".index(r[p]) + 1 + i % 3) % 4]
        reads.append("".join(r))
    write_specimen(root, "S_subs", rng, reads)
    return types.SimpleNamespace(root=root, subs=subs)


def run_errors(root, out_dir, profile_fn=profile_reference, fastq=None, status=0, twins=TWINS, **options):
    """errors.run on the tree (or one file) with every output switched on; returns {output name: bytes}."""
    os.makedirs(out_dir, exist_ok=True)
    argv = ["--fastq", fastq] if fastq else ["--run-dir", root]
    argv += ["--report", os.path.join(out_dir, "errors.tsv"), "--quality", os.path.join(out_dir, "quality.tsv"),
             "--homopolymers", os.path.join(out_dir, "homopolymers.tsv"), "--reads", os.path.join(out_dir, "reads.tsv"),
             "--json", os.path.join(out_dir, "errors.json"), "--fasta", os.path.join(out_dir, "called.fasta")]
    for key, val in options.items():
        argv += ["--" + key.replace("_", "-")] + ([] if val is True else [str(val)])
    args = errors.build_parser().parse_args(argv)
    assert errors.run(args, profile_fn=profile_fn, **twins) == status
    files = {}
    for name in OUTPUTS if status == 0 else ():
        with open(os.path.join(out_dir, name), "rb") as fh:
            files[name] = fh.read()
    return files


def table_rows(data, columns):
    lines = data.decode("latin-1").splitlines()
    assert lines[0].split("\t") == list(columns)
    return [types.SimpleNamespace(**dict(zip(columns, ln.split("\t")))) for ln in lines[1:]]


@pytest.fixture(scope="module")
def default_run(plate, tmp_path_factory):
    asked = []

    def spy(reads, quals, ks, jobs, kernel_ms=None):
        asked.append((reads, quals, ks, jobs))
        return profile_reference(reads, quals, ks, jobs)
    return run_errors(plate.root, str(tmp_path_factory.mktemp("default")), profile_fn=spy), asked


def test_the_report_of_the_plate(plate, default_run):
    files, asked = default_run
    rows = {os.path.basename(r.specimen): r for r in table_rows(files["errors.tsv"], errors.COLUMNS)}
    assert list(rows) == ["S_clean.fastq", "S_noisy.fastq", "S_subs.fastq", "run"]
    assert all(r.reads == r.aligned == "30" and r.not_aligned == "0" and r.clipped == "0" for k, r in rows.items() if k != "run")
    assert rows["run"].reads == "90" and rows["run"].sequences == "3"
    # the planted rates: exactly SUBS_PER_READ substitutions per read and nothing else
    s = rows["S_subs.fastq"]
    assert s.bases == str(30 * 300) and s.sub_per_kb == f"{1000 * 30 * SUBS_PER_READ / 9000:.3f}"
    assert s.ins_per_kb == s.del_per_kb == s.other_per_kb == "0.000"      # (a substitution inside a run still shortens the run)
    assert s.identity_p5 == s.identity_p50 == s.identity_p95 == f"{297 / 300:.4f}"
    assert float(rows["S_clean.fastq"].sub_per_kb) < float(rows["S_noisy.fastq"].sub_per_kb)
    assert float(rows["S_noisy.fastq"].hp_off) > 0.05 > float(rows["S_clean.fastq"].hp_off)
    # one device call: the members of the three sequences back to back, then the three drafts, under the 0.80 limit
    (reads, quals, ks, jobs), = asked
    assert len(reads) == 93 and [n for _, _, n in jobs] == [30, 30, 30] and [d for d, _, _ in jobs] == [90, 91, 92]
    assert ks[:90] == [int(len(r) * (1 - 0.80)) for r in reads[:90]] and all(len(q) == len(r) for q, r in zip(quals, reads))
    assert reads[92] == plate.subs.encode()


def test_the_other_outputs(default_run):
    files, _ = default_run
    q = table_rows(files["quality.tsv"], errors.QUALITY_COLUMNS)
    assert [int(r.q) for r in q] == list(range(10, 41))        # clusters_utils.fastq_text: Phred 10..40, all of them met
    assert all(int(r.bases) == int(r.match) + int(r.errors) and int(r.errors) == int(r.sub_other) + int(r.inserted) for r in q)
    doc = json.loads(files["errors.json"])
    assert sum(int(r.bases) for r in q) == sum(doc["run"]["counts"][k] for k in ("match", "sub", "other", "ins_bases"))
    hp = files["homopolymers.tsv"].decode().splitlines()
    assert hp[0].split("\t") == ["true_length", "-3", "-2", "-1", "0", "+1", "+2", "+3"] and hp[8].startswith("8+\t")
    eight = [int(x) for x in hp[8].split("\t")[1:]]
    assert sum(eight) >= 90 and eight[2] >= 8                  # the planted run, a base short in a third of S_noisy's reads
    reads = table_rows(files["reads.tsv"], errors.READ_COLUMNS)
    assert len(reads) == 90 and len({r.read for r in reads}) == 90
    assert sum(int(r.sub) for r in reads if r.name == "S_subs_c1") == 30 * SUBS_PER_READ
    assert all(float(r.predicted_error_per_kb) > 0 for r in reads)
    implied = doc["implied"]
    assert "model" in implied["note"] and [p["length"] for p in implied["patterns"]] == [13, 20]
    p5 = errors.identity_percentiles([errors.identity_parts([int(getattr(r, k)) for k in errors.READ_COLUMNS[3:10]]) for r in reads], (5,))[0]
    assert implied["min_identity"] == f"{(100 * p5[0]) // p5[1] / 100:.2f}"
    for p in implied["patterns"]:
        shares = [float(p["more_than"][str(e)]) for e in range(5)]
        assert shares == sorted(shares, reverse=True) and 0 < shares[0] < 1
    assert doc["settings"]["final_min_identity"] == 0.80 and doc["summary"]["profile_calls"] == 1
    assert files["called.fasta"].count(b">") == 3


def test_a_given_min_identity_serves_the_final_alignment_too(plate, tmp_path):
    seen = []

    def spy(reads, quals, ks, jobs, kernel_ms=None):
        seen.append(ks)
        return profile_reference(reads, quals, ks, jobs)
    fastq = os.path.join(plate.root, "full", "POOL", "S_subs.fastq")
    files = run_errors(plate.root, str(tmp_path), profile_fn=spy, fastq=fastq, min_identity=0.95, pattern_lengths="7")
    assert seen[0][:30] == [int(300 * (1 - 0.95))] * 30
    doc = json.loads(files["errors.json"])
    assert doc["settings"]["final_min_identity"] == 0.95 and [p["length"] for p in doc["implied"]["patterns"]] == [7]


def test_haplotypes_run(plate, tmp_path):
    files = run_errors(plate.root, str(tmp_path), fastq=os.path.join(plate.root, "full", "POOL", "S_clean.fastq"), haplotypes=True)
    rows = table_rows(files["errors.tsv"], errors.COLUMNS)
    assert [r.reads for r in rows] == ["30", "30"]


def test_argument_errors(plate, tmp_path):
    run_errors(plate.root, str(tmp_path), status=2, pattern_lengths="0")
    run_errors(plate.root, str(tmp_path), status=2, pattern_lengths="x")
    run_errors(plate.root, str(tmp_path), status=2, pattern_lengths=",")
    run_errors(plate.root, str(tmp_path), status=2, min_identity=1.5)
    run_errors(plate.root, str(tmp_path), status=2, haplotypes=True, max_sites=0)
    run_errors(plate.root, str(tmp_path), status=1, fastq=os.path.join(plate.root, "missing.fastq"))
    with pytest.raises(SystemExit):
        errors.build_parser().parse_args(["--report", "x.tsv"])            # neither --run-dir nor --fastq
    with pytest.raises(ValueError):
        from specimux_amd import calls
        calls.cons_profile([b"ACGT"], [b"II"], [1], [(0, 0, 0)])              # a quality string of another length
