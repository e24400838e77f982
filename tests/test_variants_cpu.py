"""specimux-variants without a GPU: the decision rules over hand-made tables, and the tool end to end over synthetic
specimens with the plain-Python twins of its device calls (clusters.adjacency_oracle, cons_utils.votes_reference,
variants_utils.phase_reference)."""
import json
import os
import random
import types

import numpy as np
import pytest

from clusters_utils import fastq_text, mutate, rand_seq
from cons_utils import votes_reference
from specimux_amd import clusters, consensus, crosstalk, identify, variants
from specimux_amd.variants import Site
from test_consensus_cpu import fasta_records, run_consensus
from variants_utils import phase_reference

OUTPUTS = ("variants.fasta", "report.tsv", "report.json", "sites.tsv")


# ------------------------------------------------------------------------------------------------ the rules
def test_linked_at_the_r2_boundary():
    # 10 + 10 reads in perfect agreement: r^2 = 1
    assert variants.linked(10, 0, 0, 10, 5, 1000)
    # n11 n00 - n10 n01 = 9 * 9 - 1 * 1 = 80, margins 10 each: r^2 = 6400 / 10000 = 0.64 exactly
    assert variants.linked(9, 1, 1, 9, 5, 640) and not variants.linked(9, 1, 1, 9, 5, 641)
    # the sign is not used: the anti-diagonal table is linked as well
    assert variants.linked(1, 9, 9, 1, 5, 640) and not variants.linked(1, 9, 9, 1, 5, 641)
    # independent sites: 25 % x 25 % of 16 reads
    assert not variants.linked(1, 3, 3, 9, 5, 1) and variants.linked(1, 3, 3, 9, 5, 0)
    # an empty margin is never linked, whatever r2 asks; nor is a table below the smallest cluster
    assert not variants.linked(0, 0, 5, 5, 5, 0) and not variants.linked(5, 5, 0, 0, 5, 0)
    assert not variants.linked(0, 5, 0, 5, 5, 0) and not variants.linked(5, 0, 5, 0, 5, 0)
    assert variants.linked(2, 0, 0, 3, 5, 1000) and not variants.linked(2, 0, 0, 2, 5, 1000)


def link_table(n, entries):
    link = np.zeros((n, n, 4), dtype=np.uint32)
    for (s, t), counts in entries.items():
        link[s, t] = counts
    return link


def test_an_unlinked_indel_is_rejected_and_a_linked_one_is_not():
    sites = [Site(10, 0, 0, 5, 30, 10), Site(20, 1, 0, 1, 30, 10), Site(30, 0, 1, 2, 30, 10), Site(40, 0, 3, 5, 28, 12)]
    # sites 0 and 1 (a deletion and an insertion) at 25 %, unlinked; site 2 a substitution at 25 %, below single-share
    partners, accepted = variants.accept_sites(sites, link_table(4, {}), 40, 5, 500, 300)
    assert partners == [[], [], [], []] and accepted == [False, False, False, False]
    # the deletion at 40 is linked to the substitution at 30: both are accepted, the others stay out
    partners, accepted = variants.accept_sites(sites, link_table(4, {(2, 3): (10, 0, 2, 28)}), 40, 5, 500, 300)
    assert partners == [[], [], [3], [2]] and accepted == [False, False, True, True]
    # an indel at 50 % on its own: still rejected
    lone = [Site(10, 0, 0, 5, 20, 20), Site(20, 1, 0, 1, 20, 20)]
    assert variants.accept_sites(lone, link_table(2, {}), 40, 5, 500, 300)[1] == [False, False]


def test_a_lone_substitution_on_either_side_of_single_share():
    for n_minor, want in ((11, False), (12, True), (13, True)):   # 12 of 40 = 30 % exactly
        sites = [Site(7, 0, 2, 0, 40 - n_minor, n_minor)]
        assert variants.accept_sites(sites, link_table(1, {}), 40, 5, 500, 300)[1] == [want], n_minor
    assert variants.accept_sites([Site(7, 0, 2, 5, 28, 12)], link_table(1, {}), 40, 5, 500, 300)[1] == [False]   # a deletion
    assert variants.accept_sites([Site(7, 1, 0, 1, 28, 12)], link_table(1, {}), 40, 5, 500, 300)[1] == [False]   # an insertion


def test_a_read_that_ties_stays_unassigned_and_the_order_of_haplotypes():
    calls = [(0, 0)] * 6 + [(1, 1)] * 6 + [(0, 1)] * 2 + [(None, 1)] + [(None, None)] + [(1, None)] * 2 + [(0, 0)]
    haps, unassigned = variants.haplotypes(calls, len(calls), 5, 100)
    # (0, 1) is one step from both and (None, None) none from both: ties; (None, 1) and (1, None) join (1, 1)
    assert unassigned == [12, 13, 15]
    assert [sig for sig, _ in haps] == [(1, 1), (0, 0)]          # 9 members against 7: the larger first
    assert haps[0][1] == [6, 7, 8, 9, 10, 11, 14, 16, 17] and haps[1][1] == [0, 1, 2, 3, 4, 5, 18]
    # equal sizes: by signature
    haps, unassigned = variants.haplotypes([(1,)] * 5 + [(0,)] * 5, 10, 5, 100)
    assert [sig for sig, _ in haps] == [(0,), (1,)] and not unassigned
    # a signature below min_cluster_size, or below min_hap_share of the aligned reads, is no haplotype: its reads join
    haps, unassigned = variants.haplotypes([(0, 0)] * 6 + [(1, 1)] * 6 + [(1, 0)] * 4, 16, 5, 100)
    assert [(sig, len(who)) for sig, who in haps] == [((0, 0), 6), ((1, 1), 6)] and unassigned == [12, 13, 14, 15]
    haps, _ = variants.haplotypes([(0,)] * 50 + [(1,)] * 5, 55, 5, 100)
    assert [(sig, len(who)) for sig, who in haps] == [((0,), 55)]          # 5 of 55 is under 10 %: one haplotype, single
    haps, _ = variants.haplotypes([(0,)] * 45 + [(1,)] * 5, 50, 5, 100)
    assert [(sig, len(who)) for sig, who in haps] == [((0,), 45), ((1,), 5)]   # 5 of 50 is 10 % exactly
    assert variants.haplotypes([()] * 8, 8, 5, 100) == ([], list(range(8)))    # no accepted site


def test_member_calls_read_the_plane_bits():
    planes = np.zeros((3, 2, 2), dtype=np.uint64)
    planes[0, 0, 0], planes[0, 1, 1] = 1 | 1 << 63, 1            # site 0: members 0 and 63 minor, 64 major
    planes[2, 1, 0] = 2                                          # site 2: member 1 major
    calls = variants.member_calls(planes, [0, 2], 66)
    assert calls[0] == (1, None) and calls[1] == (None, 0) and calls[63] == (1, None) and calls[64] == (0, None)
    assert calls[65] == (None, None) and len(calls) == 66


def test_polish_from_a_given_draft():
    """drafts=: the draft is not a member and does not vote; without it the first member is the draft, as before."""
    seen = []

    def spy(reads, ks, jobs, kernel_ms=None):
        seen.append(([r.decode() for r in reads], list(jobs)))
        return votes_reference(reads, ks, jobs, kernel_ms)
    done, _ = consensus.polish([["ACGTACGTAC"] * 6], 0.8, 3, 5, spy, drafts=["ACGAACGTAC"])
    assert done == [("ACGTACGTAC", 6, 2, "converged")]
    assert seen[0] == (["ACGTACGTAC"] * 6 + ["ACGAACGTAC"], [(6, 0, 6)])
    assert seen[1][1] == [(7, 0, 6)] and seen[1][0][7] == "ACGTACGTAC"
    del seen[:]
    done, _ = consensus.polish([["ACGTACGTAC"] * 6], 0.8, 3, 5, spy)
    assert done == [("ACGTACGTAC", 6, 1, "converged")] and seen == [(["ACGTACGTAC"] * 6, [(0, 0, 6)])]


# ------------------------------------------------------------------------------------------------ the tool
def two_haplotypes(seed):
    """Two 300-nt templates that differ by two substitutions 120 nt apart, 24 + 16 reads at 5 % error, shuffled."""
    rng = random.Random(seed)
    a = rand_seq(rng, 300)
    b = list(a)
    for p in (90, 210):
        b[p] = rng.choice([c for c in "ACGT" if c != a[p]])
    b = "".join(b)
    reads = [mutate(rng, a, 0.05) for _ in range(24)] + [mutate(rng, b, 0.05) for _ in range(16)]
    rng.shuffle(reads)
    return rng, (a, b), reads


def one_template(seed):
    """One 300-nt template with an 8-base homopolymer that a quarter of the 40 reads shorten by one; 5 % error."""
    rng = random.Random(seed)
    left, right = rand_seq(rng, 146), rand_seq(rng, 146)
    base = rng.choice([c for c in "ACGT" if c != left[-1] and c != right[0]])
    full, short = left + base * 8 + right, left + base * 7 + right
    reads = [mutate(rng, short if i % 4 == 0 else full, 0.05) for i in range(40)]
    rng.shuffle(reads)
    return rng, (full,), reads


def write_specimen(root, name, rng, reads):
    pool = os.path.join(root, "full", "POOL")
    os.makedirs(pool, exist_ok=True)
    path = os.path.join(pool, name + ".fastq")
    with open(path, "w") as fh:
        fh.write(fastq_text(rng, name, reads))
    return path


def run_variants(root, out_dir, adjacency_fn, votes_fn, phase_fn, fastq=None, **options):
    """variants.run on the tree (or one file) with every output switched on; returns {output name: bytes}."""
    os.makedirs(out_dir, exist_ok=True)
    argv = ["--fastq", fastq] if fastq else ["--run-dir", root]
    argv += ["--fasta", os.path.join(out_dir, "variants.fasta"), "--report", os.path.join(out_dir, "report.tsv"),
             "--json", os.path.join(out_dir, "report.json"), "--sites", os.path.join(out_dir, "sites.tsv")]
    for key, val in options.items():
        argv += ["--" + key.replace("_", "-"), str(val)]
    args = variants.build_parser().parse_args(argv)
    assert variants.run(args, adjacency_fn=adjacency_fn, votes_fn=votes_fn, phase_fn=phase_fn) == 0
    files = {}
    for name in OUTPUTS:
        with open(os.path.join(out_dir, name), "rb") as fh:
            files[name] = fh.read()
    return files


def table_rows(data, columns):
    lines = data.decode("latin-1").splitlines()
    assert lines[0].split("\t") == list(columns)
    return [types.SimpleNamespace(**dict(zip(columns, ln.split("\t")))) for ln in lines[1:]]


def check_two_haplotypes(files, templates, name="S"):
    """Two records whose sequences are the two templates, the larger first; the four outputs agree with each other."""
    recs = fasta_records(files["variants.fasta"])
    assert [r.name for r in recs] == [f"{name}_c1_h1", f"{name}_c1_h2"]
    assert [r.seq for r in recs] == list(templates)
    assert int(recs[0].size) >= int(recs[1].size) >= 5 and int(recs[0].size) + int(recs[1].size) <= 40
    sites = [s for s in table_rows(files["sites.tsv"], variants.SITE_COLUMNS) if s.accepted == "yes"]
    assert [(s.pos, s.kind) for s in sites] == [("90", "base"), ("210", "base")]
    assert sites[0].partners == "210" and sites[1].partners == "90" and {s.clipped for s in sites} == {"-"}
    a, b = templates
    assert recs[0].sites == f"90{a[90]},210{a[210]}" and recs[1].sites == f"90{b[90]},210{b[210]}"
    rows = table_rows(files["report.tsv"], variants.COLUMNS)
    doc = json.loads(files["report.json"])
    docs = [c for s in doc["specimens"] for c in s["clusters"]]
    assert len(rows) == len(docs) == 2 and doc["summary"]["split"] == 1 and doc["summary"]["haplotypes"] == 2
    for rec, row, c in zip(recs, rows, docs):
        assert rec.name == row.name == c["name"] and rec.seq == c["consensus"] and c["parent"] == f"{name}_c1"
        assert (rec.size, rec.aligned, rec.rounds, rec.sites) == (row.size, row.aligned, row.rounds, row.sites) \
            == tuple(str(c[x]) for x in ("size", "aligned", "rounds", "sites"))
        assert rec.share == row.share == f"{c['share']:.4f}" and int(row.length) == len(rec.seq) == c["length"]
    return recs


# The seeds are §15's, 1-6.  A seed on which the twin itself misses would be replaced by the next integer (at most two of
# the six) and noted here with what the twin returned.  None had to be.
SEEDS = [1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("seed", SEEDS)
def test_two_haplotypes_are_told_apart(seed, tmp_path):
    rng, templates, reads = two_haplotypes(seed)
    root = str(tmp_path / "out")
    path = write_specimen(root, "S", rng, reads)
    files = run_variants(root, str(tmp_path / "res"), clusters.adjacency_oracle, votes_reference, phase_reference)
    check_two_haplotypes(files, templates)
    # plain consensus on the same file: one cluster, whose sequence is the larger template
    plain = run_consensus(root, str(tmp_path / "plain"), clusters.adjacency_oracle, votes_reference)
    recs = fasta_records(plain["consensus.fasta"])
    assert [r.name for r in recs] == ["S_c1"] and recs[0].seq == templates[0]
    assert json.loads(plain["report.json"])["specimens"][0]["status"] == "ok"
    assert path == json.loads(files["report.json"])["specimens"][0]["specimen"]


@pytest.mark.parametrize("seed", SEEDS)
def test_a_homopolymer_error_stays_single(seed, tmp_path):
    rng, (full,), reads = one_template(seed)
    root = str(tmp_path / "out")
    write_specimen(root, "S", rng, reads)
    files = run_variants(root, str(tmp_path / "res"), clusters.adjacency_oracle, votes_reference, phase_reference)
    plain = run_consensus(root, str(tmp_path / "plain"), clusters.adjacency_oracle, votes_reference)
    assert files["variants.fasta"] == plain["consensus.fasta"]   # the single cluster's record, unchanged
    recs = fasta_records(files["variants.fasta"])
    assert [r.name for r in recs] == ["S_c1"] and len(recs[0].seq) in (len(full) - 1, len(full))   # a run of 7 or of 8
    doc = json.loads(files["report.json"])
    assert doc["summary"]["split"] == 0 and doc["summary"]["phase_calls"] == 1
    assert doc["specimens"][0]["clusters"] == json.loads(plain["report.json"])["specimens"][0]["clusters"]
    # the shortened run is seen -- a deletion or a missing insertion in the run, at a quarter of the reads -- and rejected
    sites = table_rows(files["sites.tsv"], variants.SITE_COLUMNS)
    run_sites = [s for s in sites if 145 <= int(s.pos) <= 154 and ("-" in (s.major, s.minor) or s.kind == "insertion")]
    assert run_sites and all(s.accepted == "no" for s in sites)
    rows = table_rows(files["report.tsv"], variants.COLUMNS)
    assert [(r.name, r.haplotype, r.sites) for r in rows] == [("S_c1", "-", "-")]


def test_json_feeds_crosstalk_and_identify(tmp_path):
    """A tree of a split specimen and a single one: the loaders behind crosstalk --consensus and identify --consensus
    read the tool's JSON as it is."""
    root = str(tmp_path / "out")
    rng, templates, reads = two_haplotypes(1)
    two = write_specimen(root, "S_two", rng, reads)
    rng, (full,), reads = one_template(1)
    one = write_specimen(root, "S_one", rng, reads)
    files = run_variants(root, str(tmp_path / "res"), clusters.adjacency_oracle, votes_reference, phase_reference)
    path = str(tmp_path / "res" / "report.json")
    refs = crosstalk.refs_from_consensus(path, [one, two])
    assert [(r.name, r.specimen, r.file, r.seq) for r in refs] == [("S_one_c1", "S_one", 0, full),
                                                                    ("S_two_c1_h1", "S_two", 1, templates[0]),
                                                                    ("S_two_c1_h2", "S_two", 1, templates[1])]
    queries = identify.queries_from_consensus(path)
    assert [(q.ref, q.seq) for q in queries] == [(r.name, r.seq) for r in refs]
    assert [r.name for r in fasta_records(files["variants.fasta"])] == [r.name for r in refs]


def test_clipped_sites_are_reported(tmp_path):
    root = str(tmp_path / "out")
    rng, templates, reads = two_haplotypes(2)
    write_specimen(root, "S", rng, reads)
    files = run_variants(root, str(tmp_path / "res"), clusters.adjacency_oracle, votes_reference, phase_reference, max_sites=1)
    sites = table_rows(files["sites.tsv"], variants.SITE_COLUMNS)
    assert [(s.pos, s.clipped, s.accepted) for s in sites] == [("90", "clipped", "yes")]   # 40 % alone: above single-share
    args = variants.build_parser().parse_args(["--run-dir", root, "--max-sites", "65"])
    assert variants.run(args, phase_fn=phase_reference) == 2
