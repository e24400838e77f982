"""specimine --run-dir without a GPU: specimen discovery, the argument rules, the skip-and-continue messages and exit
status, the shard planner and the budget planner."""
import logging
import os
import random

import pytest

from specimux_amd import specimine, synth


def touch(path, text=""):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text)


def rec(i, seq="ACGTACGTAC"):
    return f"@r{i} d\n{seq}\n+\n{'I' * len(seq)}\n"


def test_discovery_both_levels(tmp_path):
    root = str(tmp_path)
    for rel in ["full/P1/A.fastq", "full/P1/sample_B.fastq", "full/P1/A.fastq.mined", "full/P1/primers.fasta",
                "full/P1/primers.txt", "full/P1/X-Y/A.fastq", "full/P1/X-Y/A.fastq.mined", "full/P1/X-Y/primers.fasta",
                "full/P1/X-Y/sample_C.fastq", "full/P0/D.fastq", "full/P0/U-V/D.fastq", "full/P1/subsample/E.fastq",
                "full/P1/X-Y/subsample/F.fastq", "subsample/P1/G.fastq", "subsample/P1/X-Y/G.fastq",
                "partial/P1/X-Y/barcode_fwd_AAA.fastq", "full/P1/notes.txt"]:
        touch(os.path.join(root, rel))
    pool = [os.path.relpath(p, root) for p in specimine.discover_specimens(root, "pool")]
    assert pool == ["full/P0/D.fastq", "full/P1/A.fastq", "full/P1/sample_B.fastq"]
    pair = [os.path.relpath(p, root) for p in specimine.discover_specimens(root, "primer-pair")]
    assert pair == ["full/P0/U-V/D.fastq", "full/P1/X-Y/A.fastq", "full/P1/X-Y/sample_C.fastq"]
    assert [specimine.extract_specimen_id(p) for p in pool] == ["D", "A", "B"]
    assert specimine.discover_specimens(str(tmp_path / "nothing"), "pool") == []
    with pytest.raises(ValueError):
        specimine.discover_specimens(root, "primer")


def test_argument_rules():
    a = specimine.parse_arguments(["--index", "i.txt", "--run-dir", "out"])
    assert a.run_dir == "out" and a.fastq is None and a.level == "pool"
    assert not a.partial_forward and not a.no_partial_reverse and a.min_identity == 0.85
    a = specimine.parse_arguments(["--index", "i.txt", "--run-dir", "out", "--level", "primer-pair", "--partial-forward",
                                   "--no-partial-reverse", "--min-identity", "0.5"])
    assert a.level == "primer-pair" and a.partial_forward and a.no_partial_reverse and a.min_identity == 0.5
    assert specimine.parse_arguments(["--index", "i.txt", "--fastq", "f.fastq"]).run_dir is None
    for argv in (["--index", "i.txt"], ["--index", "i.txt", "--fastq", "f.fastq", "--run-dir", "out"],
                 ["--index", "i.txt", "--run-dir", "out", "--level", "pair"], ["--run-dir", "out"]):
        with pytest.raises(SystemExit) as e:
            specimine.parse_arguments(argv)
        assert e.value.code == 2


def test_read_index_first_row_wins(tmp_path):
    idx = tmp_path / "idx.txt"
    idx.write_text("SampleID\tPrimerPool\tFwIndex\tFwPrimer\tRvIndex\tRvPrimer\n"
                   "S1\tP\tacgt\tF\tttgg\tR\nS1\tP\tCCCC\tF\tGGGG\tR\nshort\tP\tAAA\nS2\tP\tAAAA\tF\tCCCC\tR\n")
    table = specimine.read_index(str(idx))
    assert table == {"S1": ("ACGT", "TTGG"), "S2": ("AAAA", "CCCC")}
    for sid in ("S1", "S2", "short", "S9"):
        assert specimine.find_barcodes(sid, str(idx)) == table.get(sid, (None, None))


def skip_tree(root):
    """Four specimens: ok, no index row, no partial file selected, empty full file."""
    touch(os.path.join(root, "specimens.txt"), "SampleID\tPrimerPool\tFwIndex\tFwPrimer\tRvIndex\tRvPrimer\n"
          "OK\tP\tAAAA\tF\tCCCC\tR\nNOPART\tP\tGGGG\tF\tTTTT\tR\nEMPTY\tP\tAAAA\tF\tCCCC\tR\n")
    touch(os.path.join(root, "full/P/OK.fastq"), rec(0))
    touch(os.path.join(root, "full/P/NOINDEX.fastq"), rec(1))
    touch(os.path.join(root, "full/P/NOPART.fastq"), rec(2))
    touch(os.path.join(root, "full/P/EMPTY.fastq"))
    touch(os.path.join(root, "partial/P/F-R/barcode_rev_CCCC.fastq"), rec(3))


def test_skips_logged_like_the_single_cli(tmp_path, caplog, monkeypatch):
    root = str(tmp_path)
    skip_tree(root)
    index = os.path.join(root, "specimens.txt")
    calls = []
    # the device part is not run here: record the planned jobs instead
    monkeypatch.setattr(specimine, "_mine_call", lambda jobs, kernel_ms=None: calls.append(jobs) or
                        [None if os.path.getsize(j.fastq) == 0 else 0 for j in jobs])
    single = {}
    for sid in ("NOINDEX", "NOPART"):
        caplog.clear()
        with pytest.raises(SystemExit) as e, caplog.at_level(logging.INFO):
            specimine.plan_job(index, os.path.join(root, "full", "P", f"{sid}.fastq"))
        assert e.value.code == 1
        single[sid] = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING]
    caplog.clear()
    with caplog.at_level(logging.INFO):
        res = specimine.mine_run(root, index)
    msgs = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING]
    for sid in ("NOINDEX", "NOPART"):
        assert single[sid] and all(m in msgs for m in single[sid])
    assert "Could not find specimen NOINDEX in index file" in msgs
    assert "No partial match files found or selected" in msgs
    assert [os.path.basename(j.fastq) for c in calls for j in c] == ["EMPTY.fastq", "OK.fastq"]
    assert res == {"specimens": 4, "planned": 2, "mined": 1, "skipped": 3, "reads": 0}


def test_exit_status(tmp_path, monkeypatch):
    root = str(tmp_path)
    skip_tree(root)
    os.remove(os.path.join(root, "full/P/OK.fastq"))
    os.remove(os.path.join(root, "full/P/EMPTY.fastq"))
    index = os.path.join(root, "specimens.txt")
    assert specimine.mine_run(root, index)["planned"] == 0
    monkeypatch.setattr(specimine, "_mine_call", lambda jobs, kernel_ms=None: [0 for _ in jobs])
    monkeypatch.setattr(specimine, "run_main", lambda args: 1 if specimine.mine_run(args.run_dir, args.index)["planned"] == 0 else 0)
    with pytest.raises(SystemExit) as e:
        specimine.main(["--index", index, "--run-dir", root])
    assert e.value.code == 1
    skip_tree(root)
    specimine.main(["--index", index, "--run-dir", root])    # one specimen planned: no exit


def shard_items(rng, n, n_files, share):
    items = []
    for i in range(n):
        files = [f"rev_{i}"]
        if rng.random() < share:
            files.append(f"fwd_{rng.randrange(n_files)}")
        items.append((rng.randint(1, 1000) * rng.randint(1, 1000), files))
    return items


@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("seed", range(6))
def test_shard_planner(world, seed):
    rng = random.Random(seed)
    items = shard_items(rng, rng.choice([1, 5, 40, 300]), rng.choice([1, 4, 32]), rng.choice([0.0, 0.7, 1.0]))
    shards = specimine.plan_shards(items, world)
    assert len(shards) == world
    flat = sorted(i for s in shards for i in s)
    assert flat == list(range(len(items)))                       # every specimen exactly once
    assert shards == specimine.plan_shards(list(items), world)  # deterministic
    total = sum(w for w, _ in items)
    bound = total / world + max(w for w, _ in items)
    assert max(sum(items[i][0] for i in s) for s in shards) <= bound


def test_shard_planner_keeps_shared_files_together():
    # 8 plate rows of 12 specimens, each row sharing one forward file; equal work: every row fits one rank of 8
    items = [(100, [f"rev_{i}", f"fwd_{i // 12}"]) for i in range(96)]
    for world in (1, 2, 8):
        shards = specimine.plan_shards(items, world)
        owner = {f"fwd_{i // 12}": r for r, s in enumerate(shards) for i in s}
        for r, s in enumerate(shards):
            assert all(owner[f"fwd_{i // 12}"] == r for i in s)
        assert max(map(len, shards)) == min(map(len, shards)) == 96 // world
    # one file shared by everything would put all work on one rank: it is split instead
    items = [(100, [f"rev_{i}", "fwd_all"]) for i in range(16)]
    shards = specimine.plan_shards(items, 8)
    assert [len(s) for s in shards] == [2] * 8


@pytest.mark.parametrize("seed", range(5))
def test_budget_planner(seed):
    rng = random.Random(seed)
    n = rng.choice([1, 7, 60])
    fsize = {f"p{j}": rng.randint(10, 5000) for j in range(rng.choice([1, 5, 20]))}
    items = [(rng.randint(10, 3000), [(f, fsize[f]) for f in rng.sample(sorted(fsize), rng.randint(1, min(3, len(fsize))))])
             for _ in range(n)]
    for budget in (1, 2000, 10000, 10 ** 9):
        calls = specimine.plan_calls(items, budget)
        assert sorted(i for c in calls for i in c) == list(range(n))
        for c in calls:
            if len(c) > 1:
                assert specimine.call_cost(items, c) <= budget
        if budget == 10 ** 9:
            assert len(calls) == 1
        if budget == 1:
            assert len(calls) == n


def test_budget_planner_groups_shared_files():
    items = [(100, [(f"fwd_{i % 3}", 1000), (f"rev_{i}", 50)]) for i in range(12)]
    calls = specimine.plan_calls(items, 100 * 4 + 50 * 4 + 1000)
    assert len(calls) == 3 and all({i % 3 for i in c} == {c[0] % 3} for c in calls)


def test_run_tree_with_shared_barcodes(tmp_path):
    ids = synth.write_mine_tree(str(tmp_path), n_specimens=6, n_full=2, n_partial=3, length=60, seed=3, fwd_groups=2,
                                pairs=("P1-P2", "P1-P3"))
    fwd = sorted(os.listdir(tmp_path / "partial" / "POOL" / "P1-P2"))
    assert len([f for f in fwd if f.startswith("barcode_fwd_")]) == 2
    assert len([f for f in fwd if f.startswith("barcode_rev_")]) == 6
    with open(tmp_path / "partial" / "POOL" / "P1-P2" / [f for f in fwd if f.startswith("barcode_fwd_")][0]) as fh:
        assert fh.read().count("\n+\n") == 3 * 3
    table = specimine.read_index(str(tmp_path / "specimens.txt"))
    assert len({table[s][0] for s in ids}) == 2
    jobs = [specimine.plan_job(str(tmp_path / "specimens.txt"), p, True)
            for p in specimine.discover_specimens(str(tmp_path), "pool")]
    assert [len(j.partial_files["forward"]) for j in jobs] == [2] * 6
