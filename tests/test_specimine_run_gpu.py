"""specimine at run scale on the GPU: smx_mine_best_identity against a host reduction of smx_mine_distances bit for
bit, and --run-dir / mine_run against one single-file CLI run per specimen (whole trees, a small budget, shards)."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from specimux_amd import _lib, calls, specimine, synth

pytestmark = pytest.mark.gpu


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, rate, alphabet="ACGT"):
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


def best_both(queries, ks, targets, jobs):
    """(host best, device best) of one job set.  Host: the reference's expression, 1.0 - d / m in float64 over
    smx_mine_distances' matrix, with d != -1, identity >= min_identity and identity > 0, the maximum per (job, target)
    starting at 0.  Device: smx_mine_best_identity.  Each output is filled with a sentinel first."""
    lib = _lib.load()
    qb = [q.encode("latin-1") for q in queries]
    tb = [t.encode("latin-1") for t in targets]
    qoff, toff = calls.offsets(qb), calls.offsets(tb)
    jarr = np.array(jobs, dtype=_lib.MINE_JOB_DTYPE)
    karr = np.array(ks, dtype=np.int32)
    n_out = int(jarr["nt"].sum()) if len(jobs) else 0
    n_dist = int((jarr["nq"].astype(np.int64) * jarr["nt"]).sum()) if len(jobs) else 0
    args = (b"".join(qb), _lib.ptr(qoff), len(qb), _lib.ptr(karr), b"".join(tb), _lib.ptr(toff), len(tb), _lib.ptr(jarr),
            len(jobs))
    dist = np.full(max(n_dist, 1), -7, dtype=np.int32)
    _lib.check(lib.smx_mine_distances(*args, _lib.ptr(dist), None))
    best = np.full(max(n_out, 1), np.nan)
    _lib.check(lib.smx_mine_best_identity(*args, _lib.ptr(best), None))
    m = np.array([len(q) for q in qb], dtype=np.float64)
    host, at = [], 0
    for q0, nq, t0, nt, mi in jobs:
        d = dist[at:at + nq * nt].reshape(nq, nt)
        at += nq * nt
        identity = 1.0 - d / m[q0:q0 + nq, None]
        ok = (d != -1) & (identity >= mi) & (identity > 0)
        host.append(np.where(ok, identity, 0.0).max(axis=0, initial=0.0))
    return (np.concatenate(host) if host else np.zeros(0)), best[:n_out]


def assert_same(queries, ks, targets, jobs):
    want, got = best_both(queries, ks, targets, jobs)
    bad = np.nonzero(want.view(np.uint64) != got.view(np.uint64))[0]
    assert bad.size == 0, f"{bad.size} of {want.size} differ: {[(float(want[i]), float(got[i])) for i in bad[:10]]}"
    return want


def test_best_random_overlapping_jobs():
    rng = random.Random(41)
    base = [rand_seq(rng, rng.randrange(40, 400)) for _ in range(20)]
    queries = [mutate(rng, rng.choice(base), rng.uniform(0, 0.1)) for _ in range(300)]
    ks = [rng.choice([-1, len(q), int(0.1 * len(q)), int(0.25 * len(q)), rng.randrange(0, len(q) + 1)]) for q in queries]
    targets = [mutate(rng, rng.choice(base), rng.uniform(0, 0.2)) if rng.random() < 0.85 else rand_seq(rng, rng.randrange(0, 300))
               for _ in range(1500)]
    jobs = [(0, 0, 0, 5, 0.5), (3, 2, 10, 0, 0.5), (0, 40, 0, 300, 0.8), (20, 30, 150, 290, 0.7), (0, 300, 0, 1500, 0.85),
            (200, 12, 500, 140, 0.0), (100, 5, 1200, 300, 0.0)]
    while len(jobs) < 600:
        q0, t0 = rng.randrange(300), rng.randrange(1500)
        jobs.append((q0, rng.randint(0, min(8, 300 - q0)), t0, rng.randint(0, min(260, 1500 - t0)),
                     rng.choice([0.0, 0.5, 0.8, 0.85, 0.9, 1.0])))
    jobs.append((299, 1, 1499, 0, 0.5))
    want = assert_same(queries, ks, targets, jobs)
    assert (want > 0).sum() > 1000 and (want == 0).sum() > 1000


def test_best_empty_targets_and_empty_jobs():
    rng = random.Random(42)
    q = rand_seq(rng, 150)
    targets = ["", mutate(rng, q, 0.05), "", q[:20], ""]
    want = assert_same([q, q[:70]], [-1, 10], targets, [(0, 2, 0, 5, 0.0), (0, 1, 0, 1, 0.0), (1, 1, 4, 1, 0.0)])
    assert want[0] == 0.0 and want[1] > 0.9     # an empty target costs the whole query: identity 0
    want, got = best_both([q], [5], ["", ""], [(0, 0, 0, 2, 0.0), (0, 1, 0, 0, 0.0)])
    assert want.size == got.size == 2 and not got.any()
    want, got = best_both([q], [5], [], [])
    assert got.size == 0
    want, got = best_both([q], [5], [q], [(0, 1, 1, 0, 0.0)])
    assert got.size == 0


def test_best_every_register_class_and_generic():
    rng = random.Random(43)
    queries, ks, targets, jobs = [], [], [], []
    for m in (1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2100):
        q = rand_seq(rng, m, rng.choice(["ACGT", "ACGTN"]))
        tl = [mutate(rng, q, rng.uniform(0, 0.3)) for _ in range(rng.choice([1, 70, 129]))] + [rand_seq(rng, m)]
        jobs.append((len(queries), 1, len(targets), len(tl), rng.choice([0.0, 0.7, 0.85])))
        queries.append(q)
        ks.append(rng.choice([-1, int(0.3 * m), int(0.15 * m)]))
        targets.extend(tl)
    jobs.append((0, len(queries), 0, len(targets), 0.5))      # every class against every target in one job
    want = assert_same(queries, ks, targets, jobs)
    assert (want > 0).sum() > 100


def test_best_thresholds_at_the_edges():
    # the pinned case: m = 5, min_identity 0.2, k = int(5 * 0.8) = 4; d = 4 is within k but identity 0.19999999999999996
    q = "ACGTA"
    k = specimine.max_distance(5, 0.2)
    assert k == 4
    targets = ["TTTTT", "ACGTA", "ACGTT", "AGGTT", "CCCCC", "GGTAC"]
    want = assert_same([q], [k], targets, [(0, 1, 0, len(targets), 0.2), (0, 1, 0, len(targets), 0.19999999999999996),
                                           (0, 1, 0, len(targets), 0.6), (0, 1, 0, len(targets), 1.0)])
    assert want[1] == 1.0 and want[len(targets) + 1] == 1.0
    # min_identity exactly at an identity of the job, and one ulp on either side
    rng = random.Random(44)
    queries = [rand_seq(rng, rng.randrange(50, 300)) for _ in range(20)]
    targets = [mutate(rng, rng.choice(queries), rng.uniform(0, 0.2)) for _ in range(200)]
    jobs = []
    for i, q in enumerate(queries):
        for e in (0.8, 0.9):
            mi = 1 - int(len(q) * (1 - e)) / len(q)
            for v in (mi, float(np.nextafter(mi, 0.0)), float(np.nextafter(mi, 2.0))):
                jobs.append((i, 1, 0, 200, v))
    assert_same(queries, [specimine.max_distance(len(q), 0.8) for q in queries], targets, jobs)


def test_best_many_queries_on_one_target():
    """Thousands of qualifying pairs raise the same few best slots at once: the atomic max must keep the largest."""
    rng = random.Random(45)
    t = rand_seq(rng, 600)
    queries = [mutate(rng, t, rng.uniform(0, 0.15)) for _ in range(3000)]
    targets = [t, mutate(rng, t, 0.02), t[:300]]
    jobs = [(0, 3000, 0, 3, 0.0), (0, 3000, 0, 1, 0.5), (1000, 2000, 1, 2, 0.8)]
    want = assert_same(queries, [-1] * 3000, targets, jobs)
    assert (want[:5] > 0).all() and want[5] == 0.0   # half a target's length: identity <= 0.5 < 0.8


# ------------------------------------------------------------------------------------------------ whole runs
def single_runs(fastqs, index, pf, npr, mi):
    """{fastq: .mined text} of one single-file CLI run per specimen; the .mined files are removed again."""
    out = {}
    for f in fastqs:
        argv = ["--index", index, "--fastq", f, "--min-identity", repr(mi)]
        if pf:
            argv.append("--partial-forward")
        if npr:
            argv.append("--no-partial-reverse")
        try:
            specimine.main(argv)
        except SystemExit as e:
            assert e.code == 1
            continue
        with open(f + ".mined", encoding="latin-1") as fh:
            out[f] = fh.read()
        os.remove(f + ".mined")
    return out


def mined_files(root):
    got = {}
    for d, _, names in os.walk(os.path.join(root, "full")):
        for n in names:
            if n.endswith(".mined"):
                p = os.path.join(d, n)
                with open(p, encoding="latin-1") as fh:
                    got[p[:-len(".mined")]] = fh.read()
                os.remove(p)
    return got


def shared_tree(root):
    synth.write_mine_tree(root, n_specimens=10, n_full=4, n_partial=8, length=300, seed=12, fwd_groups=3,
                          pairs=("P1-P2", "P1-P3"))
    return os.path.join(root, "specimens.txt")


@pytest.mark.parametrize("level", ["pool", "primer-pair"])
def test_run_dir_golden_tree(tmp_path, monkeypatch, level):
    shutil.copytree(os.path.join(GOLDEN, "expected_output"), tmp_path / "out")
    shutil.copy(os.path.join(GOLDEN, "specimens.txt"), tmp_path / "out" / "specimens.txt")
    monkeypatch.chdir(tmp_path / "out")
    fastqs = specimine.discover_specimens(".", level)
    assert len(fastqs) == 3
    for pf, npr, mi in ((True, False, 0.3), (False, False, 0.85), (True, True, 0.5)):
        want = single_runs(fastqs, "specimens.txt", pf, npr, mi)
        argv = ["--index", "specimens.txt", "--run-dir", ".", "--level", level, "--min-identity", repr(mi)]
        if pf:
            argv.append("--partial-forward")
        if npr:
            argv.append("--no-partial-reverse")
        if want:
            specimine.main(argv)
        else:
            with pytest.raises(SystemExit) as e:
                specimine.main(argv)
            assert e.value.code == 1
        assert mined_files(".") == want


@pytest.mark.parametrize("level", ["pool", "primer-pair"])
def test_run_dir_shared_barcodes(tmp_path, level):
    root = str(tmp_path)
    index = shared_tree(root)
    fastqs = specimine.discover_specimens(root, level)
    assert len(fastqs) == (10 if level == "pool" else 20)
    for pf, npr, mi in ((True, False, 0.8), (False, False, 0.85), (True, True, 0.0)):
        want = single_runs(fastqs, index, pf, npr, mi)
        res = specimine.mine_run(root, index, level, pf, npr, mi)
        assert mined_files(root) == want
        assert res["mined"] == len(want) and res["reads"] == sum(v.count("\n+\n") for v in want.values())
    assert sum(v.count("\n+\n") for v in want.values()) > 0


def test_small_budget_forces_several_calls(tmp_path):
    root = str(tmp_path)
    index = shared_tree(root)
    fastqs = specimine.discover_specimens(root, "pool")
    want = single_runs(fastqs, index, True, False, 0.8)
    ms = []
    specimine.mine_run(root, index, "pool", True, False, 0.8, budget=60_000, kernel_ms=ms)
    assert len(ms) >= 3
    assert mined_files(root) == want


def test_shards_together_equal_world_1(tmp_path, monkeypatch):
    root = str(tmp_path)
    index = shared_tree(root)
    specimine.mine_run(root, index, "primer-pair", True, False, 0.8)
    want = mined_files(root)
    assert len(want) == 20
    for world in (2, 8):
        got, total = {}, 0
        for rank in range(world):
            res = specimine.mine_run(root, index, "primer-pair", True, False, 0.8, rank=rank, world=world)
            mine = mined_files(root)
            assert not set(mine) & set(got)          # no file has two writers
            got.update(mine)
            total += res["mined"]
        assert got == want and total == 20


def test_two_process_launch(tmp_path):
    root = str(tmp_path)
    index = shared_tree(root)
    specimine.mine_run(root, index, "pool", True, False, 0.8)
    want = mined_files(root)
    env = dict(os.environ, PYTHONPATH=REPO, MASTER_PORT=str(29500 + os.getpid() % 1000))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2",
                        "--master-port", env["MASTER_PORT"], "-m", "specimux_amd.specimine", "--index", index,
                        "--run-dir", root, "--partial-forward", "--min-identity", "0.8"],
                       env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert mined_files(root) == want
    assert "Mined 10 specimen(s), skipped 0 of 10" in r.stderr
