"""specimine on the GPU: the mining kernel's HW distances against the O(m*n) oracle DP, and whole .mined files
against a plain-Python restatement of the reference loop (specimine.py:197-257) over oracle distances."""
import glob
import os
import random
import shutil

import numpy as np
import pytest

from conftest import GOLDEN
from oracle.edlib_semantics import HW, align_c
from specimux_amd import _lib, specimine, synth

pytestmark = pytest.mark.gpu


def oracle_dist(q, t, k):
    return align_c(q, t, HW, k, iupac=False)["editDistance"]


def kernel_dists(pairs):
    """[(query, target, k)] -> kernel distances, one smx_mine_distances call (one job per pair group of a query/k)."""
    lib = _lib.load()
    groups = {}
    for i, (q, t, k) in enumerate(pairs):
        groups.setdefault((q, k), []).append(i)
    queries, ks, targets, jobs, order = [], [], [], [], []
    for (q, k), idx in groups.items():
        jobs.append((len(queries), 1, len(targets), len(idx), 0.0))
        queries.append(q.encode("latin-1"))
        ks.append(k)
        targets.extend(pairs[i][1].encode("latin-1") for i in idx)
        order.extend(idx)
    qoff = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.uint64)
    toff = np.concatenate([[0], np.cumsum([len(t) for t in targets])]).astype(np.uint64)
    jarr = np.array(jobs, dtype=_lib.MINE_JOB_DTYPE)
    dist = np.full(len(pairs), -7, dtype=np.int32)
    _lib.check(lib.smx_mine_distances(b"".join(queries), _lib.ptr(qoff), len(queries), _lib.ptr(np.array(ks, np.int32)),
                                      b"".join(targets), _lib.ptr(toff), len(targets), _lib.ptr(jarr), len(jobs),
                                      _lib.ptr(dist), None))
    out = np.empty(len(pairs), dtype=np.int64)
    out[np.array(order)] = dist
    return out


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


def check(pairs):
    got = kernel_dists(pairs)
    bad = [(len(q), len(t), k, int(g), oracle_dist(q, t, k)) for (q, t, k), g in zip(pairs, got)
           if g != oracle_dist(q, t, k)]
    assert not bad, f"{len(bad)} of {len(pairs)} pairs differ (m, n, k, kernel, oracle): {bad[:10]}"


def test_distances_lengths_and_limits():
    rng = random.Random(11)
    pairs = []
    for m in (1, 2, 63, 64, 65, 127, 128, 129, 200, 600, 1025, 1500, 4097, 5000):
        ks = sorted({0, min(3, m), int(0.15 * m), m, m + 5, -1})
        reps = 6 if m <= 1500 else 1
        for _ in range(reps):
            alphabet = rng.choice(["ACGT", "ACGT", "ACGTNRY", "ACGTacgtN"])
            q = rand_seq(rng, m, alphabet)
            for k in ks:
                kk = m if k < 0 else k
                core = mutate(rng, q, 0.1, alphabet)
                cands = [
                    core,                                                                   # about m
                    q,                                                                      # identical
                    core[:max(0, m - kk - 1 - rng.randrange(3))],                           # shorter than m - k
                    rand_seq(rng, rng.randrange(0, 40)) + core + rand_seq(rng, rng.randrange(0, 40)),
                    "",                                                                     # empty target
                ]
                if m <= 1500:
                    cands.append(rand_seq(rng, rng.randrange(m, 2 * m + 40)) + core + rand_seq(rng, m // 2))  # much longer
                    cands.append(rand_seq(rng, m + rng.randrange(-3, 30), alphabet))          # unrelated
                for t in cands:
                    pairs.append((q, t, k))
    assert len(pairs) > 1000
    check(pairs)


def test_distances_long_query():
    rng = random.Random(12)
    q = rand_seq(rng, 16400)
    t = rand_seq(rng, 50) + mutate(rng, q, 0.05) + rand_seq(rng, 50)
    check([(q, t, int(0.15 * len(q))), (q, t, 10)])


def test_distances_one_query_many_targets_and_many_queries_one_target():
    rng = random.Random(13)
    q = rand_seq(rng, 300)
    targets = [mutate(rng, q, rng.uniform(0, 0.3)) if i % 3 else rand_seq(rng, rng.randrange(250, 350))
               for i in range(1000)]
    check([(q, t, 45) for t in targets])
    t = rand_seq(rng, 400)
    queries = [mutate(rng, t[s:s + ln], 0.1) or "A" for s, ln in ((rng.randrange(0, 250), rng.randrange(1, 150)) for _ in range(1000))]
    check([(x, t, int(len(x) * 0.15)) for x in queries])


# ---------------------------------------------------------------------------------------- whole files
def expected_mined_text(index, fastq, partial_forward, no_partial_reverse, min_identity):
    """The reference's mining loop restated over oracle distances, formatted as its FASTQ writer does."""
    sid = specimine.extract_specimen_id(fastq)
    b1, b2 = specimine.find_barcodes(sid, index)
    files = specimine.derive_partial_match_filenames(fastq, b1, b2)
    if not partial_forward:
        files.pop("forward", None)
    if no_partial_reverse:
        files.pop("reverse", None)
    fulls = specimine.read_fastq(fastq)
    out = []
    if not fulls:
        return ""
    for ptype, flist in files.items():
        for f in flist:
            for p in specimine.read_fastq(f):
                best = 0
                for fr in fulls:
                    k = int(len(fr.seq) * (1 - min_identity))
                    d = oracle_dist(fr.seq, p.seq, k)
                    if d != -1:
                        identity = 1 - (d / len(fr.seq))
                        if identity >= min_identity and identity > best:
                            best = identity
                if best:
                    title = f"{p.id}_mined_{ptype}_{best:.2f} {p.description} mined_{ptype} identity={best:.2f}"
                    out.append(f"@{title}\n{p.seq}\n+\n{p.quality_string}\n")
    return "".join(out)


def run_cli(fastq, index, partial_forward, no_partial_reverse, min_identity):
    argv = ["--index", index, "--fastq", fastq, "--min-identity", repr(min_identity)]
    if partial_forward:
        argv.append("--partial-forward")
    if no_partial_reverse:
        argv.append("--no-partial-reverse")
    specimine.main(argv)
    with open(fastq + ".mined", encoding="latin-1") as fh:
        return fh.read()


@pytest.mark.parametrize("min_identity", [0.85, 0.3])
def test_golden_tree_pool_level(tmp_path, monkeypatch, min_identity):
    shutil.copytree(os.path.join(GOLDEN, "expected_output"), tmp_path / "out")
    shutil.copy(os.path.join(GOLDEN, "specimens.txt"), tmp_path / "out" / "specimens.txt")
    monkeypatch.chdir(tmp_path / "out")
    fastq = "full/ITS2/TEST_SPECIMEN_001.fastq"
    files = specimine.derive_partial_match_filenames(fastq, "ATAATATTCGGCA", "AACGGCCTTGAGG")
    assert sorted(os.path.basename(os.path.dirname(f)) for f in files["forward"]) == ["gITS7-ITS4", "gITS7-unknown"]
    got = run_cli(fastq, "specimens.txt", True, False, min_identity)
    assert got == expected_mined_text("specimens.txt", fastq, True, False, min_identity)
    if min_identity < 0.5:
        assert got.count("\n+\n") > 0, "the low threshold should mine something"


def test_synthetic_tree(tmp_path):
    root = str(tmp_path)
    ids = synth.write_mine_tree(root, n_specimens=3, n_full=5, n_partial=12, length=300, seed=5,
                                pairs=("P1-P2", "P1-P3"))
    # ties between full reads of different length: a full file whose reads are one insert and its 1-nt-shorter prefix
    with open(os.path.join(root, "full", "POOL", ids[0] + ".fastq")) as fh:
        lines = fh.read().split("\n")
    s = lines[1]
    with open(os.path.join(root, "full", "POOL", ids[0] + ".fastq"), "a") as fh:
        fh.write(f"@tie_a\n{s[:-1]}\n+\n{'I' * (len(s) - 1)}\n@tie_b\n{s[:-2]}\n+\n{'I' * (len(s) - 2)}\n")
    index = os.path.join(root, "specimens.txt")
    total = 0
    for sid in ids:
        for fastq in (os.path.join(root, "full", "POOL", f"{sid}.fastq"), os.path.join(root, "full", "POOL", "P1-P2", f"{sid}.fastq")):
            for min_identity in (0.0, 0.5, 0.85, 1.0):
                for pf, npr in ((True, False), (False, False), (True, True)):
                    got = run_cli(fastq, index, pf, npr, min_identity)
                    assert got == expected_mined_text(index, fastq, pf, npr, min_identity), (fastq, min_identity, pf, npr)
                    total += got.count("\n+\n")
    assert total > 0


def test_mine_specimens_equals_one_run_per_specimen(tmp_path):
    root = str(tmp_path)
    ids = synth.write_mine_tree(root, n_specimens=6, n_full=4, n_partial=10, length=250, seed=9)
    index = os.path.join(root, "specimens.txt")
    fastqs = [os.path.join(root, "full", "POOL", f"{sid}.fastq") for sid in ids]
    single = {}
    for f in fastqs:
        single[f] = run_cli(f, index, True, False, 0.8)
        os.remove(f + ".mined")
    jobs = [specimine.plan_job(index, f, True, False, 0.8) for f in fastqs]
    specimine.mine_specimens(jobs)
    for f in fastqs:
        with open(f + ".mined", encoding="latin-1") as fh:
            assert fh.read() == single[f]
    assert sum(v.count("\n+\n") for v in single.values()) > 0
    assert glob.glob(os.path.join(root, "full", "POOL", "*.mined"))
