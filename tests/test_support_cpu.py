"""specimux-support without a GPU: the subsets and the numbers on their own, and the tool end to end over a small synthetic
plate with the plain-Python twins of its device calls (clusters.adjacency_oracle, cons_utils.votes_reference,
variants_utils.phase_reference, support_utils.resample_reference)."""
import json
import os
import random
import types

import numpy as np
import pytest

from clusters_utils import fastq_text, mutate, rand_seq
from cons_utils import votes_reference
from specimux_amd import clusters, support
from support_utils import resample_reference
from test_consensus_cpu import fasta_records, run_consensus
from test_variants_cpu import two_haplotypes, write_specimen
from variants_utils import phase_reference

# The seed of the plate's runs.  Whether the 60/40 column of S_split comes out weak is a draw: a half sample of 10 of the
# 20 reads drops the column when it holds 6 or more of the 8 reads with the other base, which 15686 of the 184756 half
# samples do (8.5 %), so about 5.4 of 64 replicates drop it and about one seed in five leaves 61 or more that keep it, the
# `need` of --min-support 0.95.  Of the seeds 1-12 two are such seeds on this plate: --seed 1 (61/64: on the threshold, not
# below it -- see test_the_seed_decides_the_subsets) and --seed 2 (62/64); the other ten leave 54 to 60.  The plate runs
# under the first of those.
SEED = 3
OUTPUTS = ("support.tsv", "support.json", "columns.tsv", "masked.fasta", "called.fasta")
TWINS = dict(adjacency_fn=clusters.adjacency_oracle, votes_fn=votes_reference, phase_fn=phase_reference)


# ------------------------------------------------------------------------------------------------ subsets and numbers
def test_need_rounds_up_in_64ths():
    assert [support.need_of(x) for x in (0.0, 0.5, 0.95, 0.96, 0.984, 0.985, 1.0)] == [0, 32, 61, 62, 63, 64, 64]


def test_subsets_have_their_size_and_depend_on_everything_in_the_key():
    base = support.subset_masks(1, "S_c1", 0, 20, 10)
    assert base.dtype == np.uint64 and base.shape == (20,)
    for b in range(64):
        assert sum((int(w) >> b) & 1 for w in base) == 10, b
    assert len({tuple((int(w) >> b) & 1 for w in base) for b in range(64)}) > 50      # the replicates differ
    for other in (support.subset_masks(2, "S_c1", 0, 20, 10), support.subset_masks(1, "S_c2", 0, 20, 10),
                  support.subset_masks(1, "S_c1", 10, 20, 10)):
        assert not np.array_equal(base, other)
    assert np.array_equal(base, support.subset_masks(1, "S_c1", 0, 20, 10))
    # the whole group where the depth does not fit; and the key is the written formula
    assert support.subset_masks(1, "S_c1", 50, 20, 20).tolist() == [2**64 - 1] * 20
    fin, g, m64 = support._fin, support.GAMMA, 2**64 - 1
    import zlib
    u = fin(fin(fin(7 + g) + zlib.crc32(b"name") + g) + 5 + g)
    assert int(support.subset_keys(7, "name", 5, 9)[63, 8]) == fin((fin((u + 63 + g) & m64) + 8 + g) & m64)
    assert fin(0 + g) == 0xE220A8397B1DCDAF                    # splitmix64's first output from state 0


def test_level_numbers_ignore_replicates_without_voters():
    agree = np.array([2**64 - 1, 2**64 - 1 - 0b101, 2**64 - 1], dtype=np.uint64)
    sub = np.full(64, 3, dtype=np.uint32)
    assert support.level_numbers(agree, sub) == ([64, 62, 64], 62)
    sub[0] = sub[63] = 0                                       # bit 0 was clear already; bit 63 now counts for nothing
    assert support.level_numbers(agree, sub) == ([62, 61, 62], 61)


# ------------------------------------------------------------------------------------------------ the tool
@pytest.fixture(scope="module")
def plate(tmp_path_factory):
    """Three specimens under root/full/POOL:
       S_noisy   30 reads of a 120-nt template at 5 % error
       S_small   6 reads of another at 2 %
       S_split   20 exact reads of a third: 12 as it is, 8 with another base at p = 40 -- a column split 60/40, every other
                 column 20/0"""
    root = str(tmp_path_factory.mktemp("plate"))
    rng = random.Random(101)
    t = rand_seq(rng, 120)
    alt = t[:40] + ("C" if t[40] != "C" else "G") + t[41:]
    split = [t] * 12 + [alt] * 8
    rng.shuffle(split)
    noisy_t, small_t = rand_seq(rng, 120), rand_seq(rng, 120)
    write_specimen(root, "S_noisy", rng, [mutate(rng, noisy_t, 0.05) for _ in range(30)])
    write_specimen(root, "S_small", rng, [mutate(rng, small_t, 0.02) for _ in range(6)])
    write_specimen(root, "S_split", rng, split)
    return types.SimpleNamespace(root=root, template=t, alt=alt)


def run_support(root, out_dir, resample_fn=resample_reference, fastq=None, status=0, **options):
    """support.run on the tree (or one file) with every output switched on; returns {output name: bytes}."""
    os.makedirs(out_dir, exist_ok=True)
    argv = ["--fastq", fastq] if fastq else ["--run-dir", root]
    argv += ["--report", os.path.join(out_dir, "support.tsv"), "--json", os.path.join(out_dir, "support.json"),
             "--columns", os.path.join(out_dir, "columns.tsv"), "--masked", os.path.join(out_dir, "masked.fasta"),
             "--fasta", os.path.join(out_dir, "called.fasta")]
    for key, val in options.items():
        argv += ["--" + key.replace("_", "-")] + ([] if val is True else [str(val)])
    args = support.build_parser().parse_args(argv)
    assert support.run(args, resample_fn=resample_fn, **TWINS) == status
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
    """The plate under --depths 3,5,10,20 and SEED, with everything the twin was asked and what it answered."""
    seen = []

    def spy(reads, ks, jobs, masks, kernel_ms=None):
        out = resample_reference(reads, ks, jobs, masks, kernel_ms)
        seen.append((list(reads), list(jobs), np.array(masks), out))
        return out
    files = run_support(plate.root, str(tmp_path_factory.mktemp("default")), resample_fn=spy, depths="3,5,10,20", seed=SEED)
    return files, seen


def test_report_of_the_plate(plate, default_run):
    files, seen = default_run
    rows = {r.name: r for r in table_rows(files["support.tsv"], support.COLUMNS)}
    assert list(rows) == ["S_noisy_c1", "S_small_c1", "S_split_c1"] and len(seen) == 1
    assert [(r.size, r.half_depth) for r in list(rows.values())[1:]] == [("6", "3"), ("20", "10")]
    for r in rows.values():                                    # a noisy read may miss the cluster, or its limit
        assert int(r.half_depth) == int(r.size) // 2 and 5 <= int(r.aligned) <= int(r.size) <= 30 and abs(int(r.length) - 120) <= 2
    assert rows["S_small_c1"].specimen.endswith("S_small.fastq")
    doc = json.loads(files["support.json"])
    assert [s["name"] for s in doc["sequences"]] == list(rows) and doc["summary"]["resample_calls"] == 1
    assert doc["settings"]["need_support"] == 61 and doc["settings"]["depths"] == [3, 5, 10, 20]
    for s in doc["sequences"]:
        r = rows[s["name"]]
        assert (r.min_support, r.whole) == (f"{s['min_support']}/64", f"{s['whole']}/64") and r.status == s["status"]
        assert r.stable_depth == ("-" if s["stable_depth"] is None else str(s["stable_depth"]))
        assert [lv["depth"] for lv in s["levels"]] == [3, 5, 10, 20] and int(r.weak_columns) == s["weak_columns"]
        # applicable: the depths below the group's size; whole is a count out of 64 there and null elsewhere
        assert [lv["whole"] is not None for lv in s["levels"]] == [d < s["size"] for d in (3, 5, 10, 20)]
        # the stable depth by its definition, from the levels
        want, ok = None, True
        for lv in reversed([lv for lv in s["levels"] if lv["whole"] is not None]):
            ok = ok and lv["whole"] >= 61
            want = lv["depth"] if ok else want
        assert s["stable_depth"] == want
    assert sum(doc["summary"][k] for k in ("solid", "weak", "unconverged")) == 3


def test_a_column_split_60_40_is_weak_and_one_20_0_is_not(plate, default_run):
    files, seen = default_run
    reads, jobs, masks, out = seen[0]
    j = 2                                                      # S_split is the third sequence of the call
    draft, r0, n = jobs[j]
    assert n == 20 and reads[draft].decode() == plate.template
    members = reads[r0:r0 + n]
    is_alt = [r.decode() == plate.alt for r in members]
    assert sum(is_alt) == 8 and all(a or r.decode() == plate.template for a, r in zip(is_alt, members))
    # what the half sample must give, from the masks alone: a replicate keeps p = 40 unless more of its ten reads carry
    # the other base than the draft's (a tie is the draft's); every other column is kept by all
    at = sum(jn for _, _, jn in jobs[:j])
    level0 = masks[0, at:at + n]
    alt_reads = [sum((int(w) >> b) & 1 for w, a in zip(level0, is_alt) if a) for b in range(64)]
    assert all(sum((int(w) >> b) & 1 for w in level0) == 10 for b in range(64))
    want = sum(1 for x in alt_reads if x <= 10 - x)
    js = out[j]
    pops = [bin(int(w)).count("1") for w in js.agree[0]]
    assert pops[40] == want and pops[:40] + pops[41:] == [64] * 120           # the twin saw both cases
    assert want < 61                                           # 8 of 20: about one half sample in twelve holds six of them
    assert js.sub_aligned[0].tolist() == [10] * 64 and js.aligned == 20
    row = {r.name: r for r in table_rows(files["support.tsv"], support.COLUMNS)}["S_split_c1"]
    assert (row.min_support, row.weak_columns, row.whole, row.status) == (f"{want}/64", "1", f"{want}/64", "weak")
    cols = [c for c in table_rows(files["columns.tsv"], support.WEAK_COLUMNS) if c.name == "S_split_c1"]
    assert [(c.pos, c.kind, c.draft, c.support, c.alt, c.alt_votes, c.votes) for c in cols] == \
        [("40", "base", plate.template[40], f"{want}/64", plate.alt[40], "8", "20")]
    masked = {r.name: r.seq for r in fasta_records(files["masked.fasta"])}["S_split_c1"]
    assert masked == plate.template[:40] + plate.template[40].lower() + plate.template[41:]


def test_masked_in_upper_case_is_the_consensus(plate, default_run, tmp_path):
    files, _ = default_run
    plain = run_consensus(plate.root, str(tmp_path / "plain"), clusters.adjacency_oracle, votes_reference)
    want = [(r.name, r.seq) for r in fasta_records(plain["consensus.fasta"])]
    assert [(r.name, r.seq.upper()) for r in fasta_records(files["masked.fasta"])] == want
    assert [(r.name, r.seq) for r in fasta_records(files["called.fasta"])] == want
    assert any(r.seq != r.seq.upper() for r in fasta_records(files["masked.fasta"]))


def test_a_group_below_every_depth_has_no_stable_depth(plate, tmp_path):
    files = run_support(plate.root, str(tmp_path / "res"), depths="10,20")
    row = {r.name: r for r in table_rows(files["support.tsv"], support.COLUMNS)}["S_small_c1"]
    assert row.size == "6" and row.stable_depth == "-"
    doc = {s["name"]: s for s in json.loads(files["support.json"])["sequences"]}["S_small_c1"]
    assert doc["levels"] == [{"depth": 10, "whole": None}, {"depth": 20, "whole": None}] and doc["stable_depth"] is None


def test_an_unconverged_cluster(plate, tmp_path):
    """--rounds 0: the called sequence is the centre read as it came, errors and all; the full vote over it calls another
    sequence, and the status says so."""
    path = os.path.join(plate.root, "full", "POOL", "S_noisy.fastq")
    files = run_support(plate.root, str(tmp_path / "res"), fastq=path, rounds=0, depths="5,10")
    rows = table_rows(files["support.tsv"], support.COLUMNS)
    assert [(r.name, r.status) for r in rows] == [("S_noisy_c1", "unconverged")] and int(rows[0].weak_columns) > 0
    assert json.loads(files["support.json"])["summary"]["unconverged"] == 1
    polished = run_support(plate.root, str(tmp_path / "res3"), fastq=path, depths="5,10")
    assert table_rows(polished["support.tsv"], support.COLUMNS)[0].status in ("solid", "weak")


def test_sixteen_depths_are_refused(plate, tmp_path, caplog):
    depths = ",".join(str(d) for d in range(2, 18))
    run_support(plate.root, str(tmp_path / "res"), status=2, depths=depths)
    assert "at most 15" in caplog.text
    run_support(plate.root, str(tmp_path / "res15"), status=0, depths=",".join(str(d) for d in range(2, 17)))
    run_support(plate.root, str(tmp_path / "bad"), status=2, depths="3,x")


def test_the_packing_into_device_calls_does_not_show(plate, default_run, tmp_path, monkeypatch):
    files, _ = default_run
    calls = []

    def counting(reads, ks, jobs, masks, kernel_ms=None):
        calls.append(len(jobs))
        return resample_reference(reads, ks, jobs, masks, kernel_ms)
    monkeypatch.setenv("SMX_CLUSTERS_BUDGET_BYTES", "1")        # a call per specimen
    small = run_support(plate.root, str(tmp_path / "small"), resample_fn=counting, depths="3,5,10,20", seed=SEED)
    assert calls == [1, 1, 1]
    del calls[:]
    monkeypatch.setenv("SMX_CLUSTERS_BUDGET_BYTES", str(1 << 30))
    large = run_support(plate.root, str(tmp_path / "large"), resample_fn=counting, depths="3,5,10,20", seed=SEED)
    assert calls == [3]
    for name in ("support.tsv", "columns.tsv", "masked.fasta", "called.fasta"):
        assert small[name] == large[name] == files[name], name


def test_the_seed_decides_the_subsets(plate, default_run, tmp_path):
    files, _ = default_run
    path = os.path.join(plate.root, "full", "POOL", "S_split.fastq")
    one = run_support(plate.root, str(tmp_path / "a"), fastq=path, depths="3,5,10,20", seed=SEED)
    again = run_support(plate.root, str(tmp_path / "b"), fastq=path, depths="3,5,10,20", seed=SEED)
    other = run_support(plate.root, str(tmp_path / "c"), fastq=path, depths="3,5,10,20", seed=1)
    assert one == again
    assert one["support.tsv"] != other["support.tsv"]
    # one file or the whole tree: the same row
    assert one["support.tsv"].splitlines()[1] == files["support.tsv"].splitlines()[3]
    # --seed 1: 61 of 64 replicates keep the split column, which is the need of 0.95 exactly: not below it, so not weak
    row = table_rows(other["support.tsv"], support.COLUMNS)[0]
    assert (row.min_support, row.weak_columns, row.status) == ("61/64", "0", "solid")
    assert len(table_rows(other["columns.tsv"], support.WEAK_COLUMNS)) == 0


def test_haplotype_names_follow_variants(tmp_path):
    rng, templates, reads = two_haplotypes(1)
    root = str(tmp_path / "out")
    write_specimen(root, "S", rng, reads)
    files = run_support(root, str(tmp_path / "res"), haplotypes=True, depths="3,5,10")
    rows = table_rows(files["support.tsv"], support.COLUMNS)
    assert [r.name for r in rows] == ["S_c1_h1", "S_c1_h2"]
    assert [r.seq for r in fasta_records(files["called.fasta"])] == list(templates)
    assert int(rows[0].size) >= int(rows[1].size) >= 5 and int(rows[0].size) + int(rows[1].size) <= 40
    # without the switch the cluster is one sequence: the larger haplotype's
    plain = run_support(root, str(tmp_path / "plain"), depths="3,5,10")
    assert [r.name for r in table_rows(plain["support.tsv"], support.COLUMNS)] == ["S_c1"]
    assert [r.seq for r in fasta_records(plain["called.fasta"])] == [templates[0]]
