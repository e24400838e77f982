"""specimux-clusters on the CPU: the clustering rule, the limits, the sampling, the status thresholds and the output files,
over hand-built graphs and the oracle twin of the device call (clusters.adjacency_oracle).  No GPU needed."""
import json
import os
import random

import numpy as np

from clusters_utils import fastq_text, rand_seq, report_rows, run_tool, write_tree
from oracle.edlib_semantics import NW, align_c
from specimux_amd import clusters, specimine


def graph(n, edges):
    a = np.zeros((n, n), dtype=bool)
    for i, j in edges:
        a[i, j] = a[j, i] = True
    return a


def check_partition(cl, n):
    assert sorted(x for c in cl for x in c) == list(range(n))             # every read in exactly one cluster
    sizes = [len(c) for c in cl]
    assert sizes == sorted(sizes, reverse=True)                           # non-increasing


def test_star_clusters_small_graphs():
    # a star around 2, a pair, a singleton
    cl = clusters.star_clusters(graph(7, [(2, 0), (2, 1), (2, 3), (4, 5)]), [1.0] * 7)
    assert cl == [[2, 0, 1, 3], [4, 5], [6]]
    check_partition(cl, 7)
    # the centre is listed first, its neighbours in index order; a neighbour's own neighbours stay behind
    cl = clusters.star_clusters(graph(5, [(3, 0), (3, 4), (4, 1), (3, 2)]), [1.0] * 5)
    assert cl == [[3, 0, 2, 4], [1]]
    # no edges: singletons in index order (equal quality), or by quality
    assert clusters.star_clusters(graph(3, []), [5.0, 5.0, 5.0]) == [[0], [1], [2]]
    assert clusters.star_clusters(graph(3, []), [5.0, 7.0, 6.0]) == [[1], [2], [0]]
    assert clusters.star_clusters(graph(0, []), []) == []
    assert clusters.star_clusters(graph(1, []), [3.0]) == [[0]]


def test_star_clusters_tie_breaks():
    path = graph(4, [(0, 1), (1, 2), (2, 3)])                             # 1 and 2 both have two neighbours
    assert clusters.star_clusters(path, [9.0, 5.0, 5.0, 9.0]) == [[1, 0, 2], [3]]      # equal quality: the lower index
    assert clusters.star_clusters(path, [9.0, 5.0, 5.5, 9.0]) == [[2, 1, 3], [0]]      # the higher quality
    # the degree counts unassigned neighbours only: after {0: 1, 2, 3} is taken, 4 (two free neighbours) beats 5
    g = graph(8, [(0, 1), (0, 2), (0, 3), (5, 1), (5, 2), (5, 6), (4, 6), (4, 7)])
    cl = clusters.star_clusters(g, [1.0] * 8)
    assert cl == [[0, 1, 2, 3], [4, 6, 7], [5]]
    check_partition(cl, 8)


def test_star_clusters_random_graphs():
    rng = random.Random(3)
    for _ in range(60):
        n = rng.randrange(1, 40)
        g = graph(n, [(i, j) for i in range(n) for j in range(i + 1, n) if rng.random() < rng.choice([0.05, 0.3])])
        q = [rng.choice([1.0, 2.0, 3.0]) for _ in range(n)]
        cl = clusters.star_clusters(g, q)
        check_partition(cl, n)
        assert cl == clusters.star_clusters(g.copy(), list(q))            # deterministic
        free = set(range(n))
        for c in cl:                                                      # restated: the rule, cluster by cluster
            deg = {x: sum(1 for y in free if g[x, y]) for x in free}
            want = min(free, key=lambda x: (-deg[x], -q[x], x))
            assert c[0] == want and c[1:] == sorted(y for y in free if g[want, y])
            free -= set(c)


def test_limit_is_the_python_expression(tmp_path):
    # 1 - 0.9 is 0.09999999999999998 in IEEE double: 300 * that is 29.999999999999993 -> 29, not 30
    assert specimine.max_distance(300, 0.9) == int(300 * (1 - 0.9)) == 29
    assert specimine.max_distance(640, 0.85) == int(640 * (1 - 0.85)) == 96
    rng = random.Random(4)
    a = rand_seq(rng, 300)
    pos = sorted(rng.sample(range(300), 30))

    def with_subs(n):
        b = list(a)
        for p in pos[:n]:
            b[p] = "ACGT"["ACGT".index(b[p]) ^ 1]
        return "".join(b)

    seen = []

    def spy(specimens, kernel_ms=None):
        seen.extend(specimens)
        return clusters.adjacency_oracle(specimens, kernel_ms)

    for nsub, want_sizes in ((29, [2]), (30, [1, 1])):                    # 30 substitutions: one past the limit of 29
        b = with_subs(nsub)
        assert align_c(a, b, NW, -1, iupac=False)["editDistance"] == nsub
        path = tmp_path / f"S{nsub}.fastq"
        path.write_text(fastq_text(rng, "S", [a, b]))
        results, _ = clusters.cluster_files([str(path)], min_identity=0.9, adjacency_fn=spy)
        assert [len(c) for c in results[0].clusters] == want_sizes
    assert all(ks == [29, 29] for _, ks in seen) and len(seen) == 2


def test_pair_limit_is_the_larger_of_the_two():
    rng = random.Random(5)
    a = rand_seq(rng, 200)
    b = a + rand_seq(rng, 25)                                             # k = 20 and 22; the distance is 25
    c = a + b[200:222]                                                    # distance 22 from a: within max(20, 22)
    adj = clusters.adjacency_oracle([([x.encode() for x in (a, b, c)], [20, 22, 22])])[0]
    assert adj.tolist() == [[False, False, True], [False, False, True], [True, True, False]]


def test_sampling_matches_subsample_top_quality(tmp_path):
    from specimux_amd.orchestration import subsample_top_quality
    rng = random.Random(6)
    full = tmp_path / "out" / "full" / "POOL"
    full.mkdir(parents=True)
    seqs = [rand_seq(rng, rng.randrange(20, 60)) for _ in range(30)]
    quals = [rng.choice("5:?DI") for _ in seqs]                           # few levels: many ties
    (full / "S.fastq").write_text(fastq_text(rng, "S", seqs, quals))
    subsample_top_quality(str(tmp_path / "out"), 11)
    kept = [r.id for r in specimine.read_fastq(str(tmp_path / "out" / "subsample" / "POOL" / "S.fastq"))]
    records = clusters.read_records(str(full / "S.fastq"))
    got = clusters.sample_top_quality([r.qual for r in records], 11)
    assert got == sorted(got) and sorted(kept) == sorted(records[i].id for i in got) and len(got) == 11
    assert clusters.sample_top_quality([r.qual for r in records], 100) == list(range(30))
    assert clusters.mean_quality("") == 0 and clusters.mean_quality("I5") == (40 + 20) / 2


def test_mixed_at_the_exact_thresholds():
    st = clusters.status_of
    assert st([36, 4], 40, 4, 0.10) == "mixed"                            # 4 reads = exactly 10 % and the minimum size
    assert st([36, 4], 40, 5, 0.10) == "ok"                               # one read short
    assert st([37, 3], 40, 3, 0.10) == "ok"                               # 7.5 %
    assert st([27, 3], 30, 3, 0.10) == "mixed"                            # 3 / 30 >= 0.1: the share, not 0.1 * 30
    assert st([40], 40, 1, 0.0) == "ok" and st([], 0, 1, 0.0) == "ok"
    assert st([20, 10, 10], 40, 5, 0.25) == "mixed" and st([20, 10, 10], 40, 5, 0.26) == "ok"


def test_read_records_keeps_the_bytes(tmp_path):
    text = b"@a one\nACGT\n+\nIIII\n\n@b\r\nAC\r\nGT\r\n+b\r\n@I\r\nII\r\n@c\nA\n+\nI"
    p = tmp_path / "x.fastq"
    p.write_bytes(text)
    recs = clusters.read_records(str(p))
    assert [(r.id, r.seq, r.qual) for r in recs] == [("a", "ACGT", "IIII"), ("b", "ACGT", "@III"), ("c", "A", "I")]
    assert b"".join(r.raw for r in recs) == text
    assert recs[1].raw == b"@b\r\nAC\r\nGT\r\n+b\r\n@I\r\nII\r\n"


def test_outputs_of_a_synthetic_tree(tmp_path):
    rng = random.Random(7)
    root = str(tmp_path / "out")
    labels = write_tree(rng, root)
    files = run_tool(root, str(tmp_path / "res"), clusters.adjacency_oracle)
    rows = report_rows(files["report.tsv"])
    by = {}
    for r in rows:
        by.setdefault(os.path.basename(r.specimen), []).append(r)
    assert sorted(by) == ["S_one.fastq", "S_six.fastq", "S_two.fastq"]    # .mined, primers.*, subsample/ are no inputs
    assert [(r.cluster, r.size, r.share, r.status) for r in by["S_one.fastq"]] == [("1", "40", "1.0000", "ok")]
    assert [(r.cluster, r.size, r.share, r.status) for r in by["S_two.fastq"]] == \
        [("1", "28", "0.7000", "mixed"), ("2", "12", "0.3000", "mixed")]
    assert [(r.cluster, r.size, r.status) for r in by["S_six.fastq"]] == [(str(i), "1", "ok") for i in range(1, 7)]
    assert all(r.reads == r.sampled for r in rows) and all(r.centre_length.isdigit() for r in rows)
    # the JSON carries the same content
    doc = json.loads(files["report.json"])
    assert doc["summary"] == {"specimens": 3, "read": 3, "failed": 0, "mixed": 1, "pairs": 780 + 780 + 15}
    flat = [(s["specimen"], str(s["reads"]), str(s["sampled"]), s["status"], str(c["rank"]), str(c["size"]),
             f"{c['share']:.4f}", c["centre"], str(c["centre_length"])) for s in doc["specimens"] for c in s["clusters"]]
    assert flat == [tuple(getattr(r, c) for c in clusters.COLUMNS) for r in rows]
    # centres: clusters of >= 5 reads, the centre read itself
    two = {r.id: r for r in clusters.read_records(os.path.join(root, "full", "POOL", "S_two.fastq"))}
    heads = [ln for ln in files["centres.fasta"].decode().splitlines() if ln.startswith(">")]
    assert [h.split()[0] for h in heads] == [">S_one_c1", ">S_two_c1", ">S_two_c2"]
    c2 = by["S_two.fastq"][1]
    assert heads[2] == f">S_two_c2 size=12 share=0.3000 read={c2.centre}"
    body = files["centres.fasta"].decode().split(heads[2] + "\n")[1].splitlines()[0]
    assert body == two[c2.centre].seq and len(body) == int(c2.centre_length)
    # split: the clusters' records byte for byte, in input order; the two templates come apart exactly
    assert sorted(f for f in files if f.startswith("split")) == [
        os.path.join("split", "POOL", n) for n in ("S_one.c1.fastq", "S_two.c1.fastq", "S_two.c2.fastq")]
    with open(os.path.join(root, "full", "POOL", "S_two.fastq"), "rb") as fh:
        src = fh.read()
    recs = clusters.read_records(os.path.join(root, "full", "POOL", "S_two.fastq"))
    for rank, label in ((1, 0), (2, 1)):
        want = b"".join(r.raw for r, x in zip(recs, labels["S_two"]) if x == label)
        assert files[os.path.join("split", "POOL", f"S_two.c{rank}.fastq")] == want
    assert b"".join(r.raw for r in recs) == src
    with open(os.path.join(root, "full", "POOL", "S_one.fastq"), "rb") as fh:
        assert files[os.path.join("split", "POOL", "S_one.c1.fastq")] == fh.read()


def test_max_reads_and_unreadable_files(tmp_path):
    rng = random.Random(8)
    root = str(tmp_path / "out")
    write_tree(rng, root)
    with open(os.path.join(root, "full", "POOL", "S_bad.fastq"), "w") as fh:
        fh.write("not a fastq file\n")
    files = run_tool(root, str(tmp_path / "res"), clusters.adjacency_oracle, max_reads=20)
    rows = report_rows(files["report.tsv"])
    assert {(os.path.basename(r.specimen), r.reads, r.sampled) for r in rows} == {
        ("S_one.fastq", "40", "20"), ("S_two.fastq", "40", "20"), ("S_six.fastq", "6", "6")}
    assert json.loads(files["report.json"])["summary"]["failed"] == 1
    # the sampled reads are the 20 best by mean quality: every read of the split files is one of them
    recs = clusters.read_records(os.path.join(root, "full", "POOL", "S_one.fastq"))
    keep = {recs[i].id for i in clusters.sample_top_quality([r.qual for r in recs], 20)}
    got = {r.id for r in clusters.read_records(str(tmp_path / "res" / "split" / "POOL" / "S_one.c1.fastq"))}
    assert got == keep
    # nothing readable at all: exit status 1
    args = clusters.build_parser().parse_args(["--fastq", os.path.join(root, "full", "POOL", "S_bad.fastq")])
    assert clusters.run(args, adjacency_fn=clusters.adjacency_oracle) == 1
    args = clusters.build_parser().parse_args(["--run-dir", str(tmp_path / "nothing")])
    assert clusters.run(args, adjacency_fn=clusters.adjacency_oracle) == 1


def test_calls_follow_the_byte_budget(tmp_path, monkeypatch):
    rng = random.Random(9)
    root = str(tmp_path / "out")
    write_tree(rng, root)
    calls = []

    def spy(specimens, kernel_ms=None):
        calls.append(len(specimens))
        return clusters.adjacency_oracle(specimens, kernel_ms)

    whole = run_tool(root, str(tmp_path / "a"), spy)
    monkeypatch.setenv("SMX_CLUSTERS_BUDGET_BYTES", "1")
    single = run_tool(root, str(tmp_path / "b"), spy)
    assert calls == [3, 1, 1, 1] and whole == single
    assert "trimmed" in clusters.build_parser().format_help()
