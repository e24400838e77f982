"""smx_inner_scan on the GPU against a numpy last-row DP written here, bit for bit (no tolerance): the window edges, the
head-window masking, alignments that straddle the margin, runs across piece boundaries, both word widths, the limits of
Q, H and the hit counter, divergent read lengths, chunking by budget, the reader-batch entry and reuse of the workspace.
The DP (tests/inner_utils.py) takes its equality relation from specimux_amd.constants."""
import numpy as np
import pytest

from inner_utils import LETTERS, expected, flat
from specimux_amd import _lib, chimera

pytestmark = pytest.mark.gpu


def check(patterns, ks, reads, margin, H, budget=0):
    bases, off = flat(reads)
    got = chimera.scan(bases, off, patterns, ks, margin, H, budget_bytes=budget)
    want = expected(patterns, ks, reads, margin, H)
    for name, g, w in zip(("nhit", "hit_dist", "hit_end"), got, want):
        bad = np.argwhere(g != w)
        assert not len(bad), (name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    return got


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n)).encode()


def plant(read, copy, end):
    """`copy` placed so that its last base is column `end`."""
    start = end - len(copy) + 1
    assert 0 <= start and end < len(read)
    return read[:start] + copy + read[end + 1:]


P22 = "CTTGGTCATTTAGAGGAAGTAA"


def test_window_edges():
    rng = np.random.default_rng(1)
    reads = []
    for n in (160, 161, 162):
        for end in (79, 80, n - 81, n - 80):
            reads.append(plant(rand_seq(rng, n), P22.encode(), end))
    nhit, dist, end = check([P22], [2], reads, 80, 4)
    # n = 162: columns 80 and 81 are internal.  A copy that ends on 79 or 82 still leaves D = 1 on the neighbouring internal
    # column (one base more or less), so all four reads have one hit; its distance tells which side of the edge the copy is
    assert nhit[8:, 0].tolist() == [1, 1, 1, 1] and dist[8:, 0, 0].tolist() == [1, 0, 0, 1]
    assert end[8:, 0, 0].tolist() == [80, 80, 81, 81]
    assert nhit[:4, 0].tolist() == [0, 0, 0, 0]           # n = 160 has no internal column


def test_head_window_copy_is_masked():
    rng = np.random.default_rng(2)
    near = P22[:10] + "A" + P22[11:]                      # distance 1 (P22[10] is T)
    read = plant(plant(rand_seq(rng, 700), P22.encode(), 50), near.encode(), 400)
    nhit, dist, end = check([P22], [2], [read], 80, 4)
    assert nhit[0, 0] == 1 and dist[0, 0, 0] == 1 and end[0, 0, 0] == 400


def test_alignment_straddling_the_margin_counts():
    rng = np.random.default_rng(3)
    read = plant(rand_seq(rng, 500), P22.encode(), 80)    # starts at column 59, inside the head window
    nhit, dist, end = check([P22], [2], [read], 80, 4)
    assert nhit[0, 0] >= 1 and dist[0, 0, 0] == 0 and end[0, 0, 0] == 80


def test_piece_boundaries():
    rng = np.random.default_rng(4)
    one = [plant(rand_seq(rng, 600), P22.encode(), 100 + i) for i in range(300)]
    check([P22, "GCATATCAATAAGCGGAGGA"], [3, 3], one, 80, 4)
    # two copies back to back: with k = 6 the runs of the two copies touch, wherever the boundary falls
    two = [plant(rand_seq(rng, 600), (P22 + P22).encode(), 130 + i) for i in range(300)]
    nhit, _, _ = check([P22], [6], two, 80, 4)
    assert (nhit[:, 0] >= 1).all()


def test_word_widths_and_limits():
    rng = np.random.default_rng(5)
    pats = [rand_seq(rng, m, "ACGT").decode() for m in (1, 31, 32, 33, 64)]
    pats[1] = "N" + pats[1][1:15] + "R" + pats[1][16:]    # degenerate letters in a 31-mer
    reads = []
    for i in range(40):
        read = rand_seq(rng, 300 + 17 * i)
        for p in pats[1:]:
            read = plant(read, p.encode(), int(rng.integers(len(p), len(read))))
        reads.append(read[:150] + b"NnRa\xff" + read[155:])
    check(pats, [0] * 5, reads, 20, 1)
    check(pats, [len(p) - 1 for p in pats], reads, 20, 8)
    check(pats[3:4], [5], reads, 0, 3)                    # Q = 1
    many = [rand_seq(rng, int(rng.integers(1, 65)), LETTERS).decode() for _ in range(128)]
    ks = [int(rng.integers(0, len(p))) for p in many]
    check(many, ks, reads[:6], 10, 2)                     # Q = 128
    for bad_q in (many + ["A"],):
        with pytest.raises(_lib.SmxError) as e:
            chimera.scan(*flat(reads[:1]), bad_q, [0] * 129, 10, 2)
        assert e.value.code == _lib.ERR_ARG


def test_more_hits_than_slots_and_counter_saturation():
    same, alt = b"A" * 20000, b"AC" * 10000
    for H in (1, 8):
        nhit, dist, end = check(["AA", "AC"], [0, 0], [same, alt], 80, H)
        assert nhit[0, 0] == 1 and nhit[0, 1] == 0         # one run over the whole interior; "AC" never within 0
        assert nhit[1, 1] == 255 and nhit[1, 0] == 0       # thousands of one-column runs
        assert (dist[1, 1] == 0).all() and end[1, 1, 0] == 81
    nhit, _, _ = check(["AC"], [0], [b"AC" * 200], 80, 8)  # more than H, fewer than 255
    assert nhit[0, 0] == 120


def test_divergent_lengths_side_by_side():
    rng = np.random.default_rng(6)
    margin = 80
    reads = [b"", rand_seq(rng, 1), rand_seq(rng, 2 * margin), rand_seq(rng, 2 * margin + 1),
             plant(plant(rand_seq(rng, 20000), P22.encode(), 9000), P22.encode(), 19900), b"", rand_seq(rng, 650)]
    reads[3] = plant(reads[3], P22.encode(), margin)
    nhit, _, end = check([P22, P22[::-1]], [2, 2], reads, margin, 4)
    assert nhit[3, 0] == 1 and end[3, 0, 0] == margin and nhit[4, 0] == 2


def test_errors_and_empty_call():
    bases, off = flat([b"ACGT" * 50])
    for pats, ks, margin, H in ((["ACGT"], [4], 0, 1), (["ACGT"], [-1], 0, 1), (["ACGT"], [1], -1, 1),
                                (["ACGT"], [1], 0, 9), (["ACGT"], [1], 0, 0), (["ACXT"], [1], 0, 1), (["A" * 65], [1], 0, 1)):
        with pytest.raises(_lib.SmxError) as e:
            chimera.scan(bases, off, pats, ks, margin, H)
        assert e.value.code == _lib.ERR_ARG, (pats, ks, margin, H)
    nhit, dist, end = chimera.scan(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), ["ACGT"], [1], 0, 2)
    assert nhit.shape == (0, 1) and dist.shape == (0, 1, 2)


def test_chunking_equals_single_chunk():
    rng = np.random.default_rng(7)
    reads = [plant(rand_seq(rng, int(rng.integers(200, 900))), P22.encode(), 150) for _ in range(400)]
    reads[137] = plant(rand_seq(rng, 15000), P22.encode(), 12345)      # larger than the budget on its own
    pats, ks = [P22, P22[::-1], "GCATATCAATAAGCGGAGGA"], [3, 3, 3]
    bases, off = flat(reads)
    whole = check(pats, ks, reads, 80, 4)
    # a 650-nt read costs about 1.2 kB here (bases, 5 units x 3 records of 24 bytes, outputs): 16 kB holds a dozen reads
    small = chimera.scan(bases, off, pats, ks, 80, 4, budget_bytes=16384)
    for a, b in zip(whole, small):
        assert np.array_equal(a, b)


def test_batch_entry_equals_flat_entry(tmp_path):
    from specimux_amd.native_io import Reader
    rng = np.random.default_rng(8)
    reads = [plant(rand_seq(rng, int(rng.integers(100, 1200))), P22.encode(), 90) for _ in range(500)]
    path = tmp_path / "reads.fastq"
    with open(path, "wb") as fh:
        for i, r in enumerate(reads):
            fh.write(b"@r%d x\n%b\n+\n%b\n" % (i, r, b"I" * len(r)))
    reader = Reader(str(path))
    batch = reader.next_batch(1000)
    assert len(batch) == 500
    pats, ks = [P22, "TTACTTCCTCTAAATGACCAAG"], [3, 3]
    got = chimera.scan_batch(batch, pats, ks, 80, 4)
    want = chimera.scan(*flat(reads), pats, ks, 80, 4)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert got[0][:, 0].sum() >= 350
    batch.close()
    reader.close()


def test_two_calls_with_different_q():
    rng = np.random.default_rng(9)
    reads = [plant(rand_seq(rng, 500), P22.encode(), 300) for _ in range(50)]
    check([P22] * 9, [2] * 9, reads, 80, 2)
    check([P22], [2], reads, 80, 2)
    check([P22, "A" * 40], [2, 3], reads, 80, 2)
