"""flank_count_kernel (specimux_amd/csrc/smx_flank.hip) at the edges of its on-chip combine, through DeviceFlank.accumulate
on synthetic device buffers: windows, lengths and hit records are built in numpy and uploaded with torch, the panel only
supplies S, Lb, k, NP and the window stride.  Table and counters are compared with tests/flank_utils.py count_reference, a
numpy restatement of tests/test_flank_gpu.py brute_force that is checked against brute_force itself here.  The keys are
steered with a Python restatement of stats_hash: into one slot of the workgroup's LDS table (more keys than a probe run
holds: the rest bypass it), into the last slots of a small global table (probing wraps), and the items past the first
and into the last, partial grid stride.  Every test asserts on the twin's own output that the edge is reached."""
import ctypes as C

import numpy as np
import pytest

from flank_utils import AMBIGUOUS, COUNTED, HITS, PRUNED, SHORT_FLANK, SHORT_READ, count_reference, make_key, stats_hash
from parity_utils import Both, tmp_panel

pytestmark = pytest.mark.gpu
LANES, LCAP, LPROBE = 256, 4096, 4        # FLANK_THREADS, FLANK_LCAP, FLANK_LPROBE (smx_flank_core.h)
_RC = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def lib():
    from specimux_amd import _lib
    lib = _lib.load()
    n = C.c_int(0)
    _lib.check(lib.smx_device_init(0, C.byref(n)))
    assert n.value >= 1
    return lib


@pytest.fixture(scope="module")
def panels(tmp_path_factory):
    from specimux_amd import synth
    from specimux_amd.demultiplex import compiled_panel
    out = {}
    for name, pan in (("c1", synth.panel_c1()), ("c3", synth.panel_c3())):
        pf, sf = tmp_panel(tmp_path_factory, pan, "flank_count_" + name)
        both = Both(pf, sf)
        out[name] = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
    assert len(out["c1"].primers) == 2 and len(out["c3"].primers) == 8
    return out


def geometry(cp):
    return cp.search_len, int(cp.desc.barcode_len_max), int(cp.desc.k_index), len(cp.primers)


def hash_np(keys):
    keys = np.asarray(keys, dtype=np.uint64)
    keys = keys ^ (keys >> np.uint64(29))
    return (keys * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32)


def keys_of_flanks(codes, matched, primer):
    """[n, W] base codes -> the keys of include/smx.h, vectorised."""
    W = codes.shape[1]
    bits = (codes.astype(np.uint64) << (2 * np.arange(W, dtype=np.uint64))[None, :]).sum(axis=1, dtype=np.uint64)
    return bits | np.uint64(W << 52 | matched << 57 | primer << 58)


class Batch:
    """n reads of 3 S bases with random ACGT windows and no hits; plant() puts a W-base flank behind a hit."""

    def __init__(self, cp, n, rng):
        from specimux_amd import _lib
        self.S, self.Lb, self.k, self.NP = geometry(cp)
        self.W = self.Lb + self.k
        self.windows = np.zeros((n, cp.window_stride), dtype=np.uint8)
        self.windows[:, :2 * self.S] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, 2 * self.S))]
        self.lens = np.full(n, 3 * self.S, dtype=np.int32)
        self.hits = np.zeros((n, 2 * self.NP), dtype=_lib.HIT_DTYPE)
        self.hits["pdist"] = -1
        self.hits["bbest"] = -1
        self.hits["nloc"] = 1

    def plant(self, i, p, e, flank, matched):
        """Hit (read i, primer p, end e) whose flank is the string `flank` (W bases): the last W positions of the end
        string's window, that is the tail window's end or the reverse complement at the head window's start."""
        S, W = self.S, self.W
        assert len(flank) == W
        if e:
            self.windows[i, 2 * S - W:2 * S] = np.frombuffer(flank.encode(), dtype=np.uint8)
        else:
            self.windows[i, :W] = np.frombuffer(flank.encode()[::-1].translate(_RC), dtype=np.uint8)
        h = self.hits[i, 2 * p + e]
        h["pdist"], h["bbest"], h["first_end"] = 0, (1 if matched else -1), (S - 1 - W) + int(self.lens[i]) - S

    def reference(self):
        return count_reference(self.S, self.Lb, self.k, self.windows, self.lens, self.hits)


def count_on_device(cp, batch, capacity, times=1):
    """[(table {key: count}, counters)] of `times` runs over the same device buffers, the table cleared in between."""
    import torch
    from specimux_amd import barcodes
    d_windows = torch.from_numpy(batch.windows).cuda()
    d_lens = torch.from_numpy(batch.lens).cuda()
    d_hits = torch.from_numpy(batch.hits.view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    fl = barcodes.DeviceFlank(cp, capacity)
    out = []
    try:
        for t in range(times):
            if t:
                fl.clear()
            fl.accumulate(None, d_windows.data_ptr(), d_lens.data_ptr(), d_hits.data_ptr(), len(batch.lens))
            keys, counts, counters = fl.read()
            assert len(set(keys.tolist())) == len(keys)                  # one slot per key
            out.append((dict(zip(keys.tolist(), counts.tolist())), counters))
    finally:
        fl.close()
    return out


def assert_equal(got, want_table, want_counters):
    table, counters = got
    assert table == want_table, (len(table), len(want_table), sorted(set(want_table) - set(table))[:5],
                                 [(key, table[key], want_table.get(key)) for key in table if table[key] != want_table.get(key)][:5])
    assert np.array_equal(counters, want_counters), (counters.tolist(), want_counters.tolist())


def letters(codes):
    return "".join("ACGT"[c] for c in codes)


def colliding_flanks(rng, W, primer, slot_mask, want, n_draw=200000):
    """`want` different W-base flanks whose keys (matched, `primer`) share one home slot under slot_mask."""
    codes = rng.integers(0, 4, (n_draw, W))
    keys = keys_of_flanks(codes, 1, primer)
    slots = hash_np(keys) & np.uint64(slot_mask)
    best = np.bincount(slots.astype(np.int64)).argmax()
    rows = np.flatnonzero(slots == np.uint64(best))
    rows = rows[np.unique(keys[rows], return_index=True)[1]][:want]
    assert len(rows) == want
    return [letters(codes[r]) for r in rows]


def test_hash_restatements_agree():
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 1 << 63, 500, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    assert hash_np(keys).tolist() == [stats_hash(key) for key in keys]
    assert stats_hash(0) == 0 and stats_hash(1) == 0x9E3779B9 and stats_hash(1 << 29) == (((1 << 29) | 1) * 0x9E3779B97F4A7C15 % (1 << 64)) >> 32


@pytest.mark.parametrize("capacity", [1 << 16, 64])
def test_keys_of_one_lds_slot_bypass_the_local_table(lib, panels, capacity):
    """12 keys with one home slot in the workgroup's LDS table fill the first workgroup's hits, at both ends: whatever the
    arrival order, four take the probe run's slots and eight go straight to the global table.  With 64 global slots they
    share their home slot there too."""
    cp = panels["c1"]
    rng = np.random.default_rng(11)
    b = Batch(cp, 300, rng)
    H = 2 * b.NP
    crowd = colliding_flanks(rng, b.W, 0, LCAP - 1, 12)
    pool = [letters(rng.integers(0, 4, b.W)) for _ in range(30)]
    first_reads = LANES // H
    for i in range(len(b.lens)):
        for e in (0, 1):
            if i < first_reads:
                b.plant(i, 0, e, crowd[(2 * i + e) % 12], 1)             # the first 256 items: one workgroup
            elif rng.integers(4):
                src = crowd if rng.integers(5) == 0 else pool
                b.plant(i, 0, e, src[int(rng.integers(len(src)))], 1)
    want, want_counters, cat, keys = b.reference()
    first = keys.reshape(-1)[:LANES][cat.reshape(-1)[:LANES] == COUNTED]
    assert len(first) == 2 * first_reads and (cat[:first_reads, 0] == COUNTED).all() and (cat[:first_reads, 1] == COUNTED).all()
    assert len(set(first.tolist())) == 12 > 2 * LPROBE
    assert len({stats_hash(key) & (LCAP - 1) for key in first.tolist()}) == 1
    home = {stats_hash(key) & (capacity - 1) for key in first.tolist()}
    assert (len(home) == 1) == (capacity == 64) and len(want) <= 42
    assert min(want[key] for key in first.tolist()) >= 10                # each of them many times
    (got,) = count_on_device(cp, b, capacity)
    assert_equal(got, want, want_counters)


def test_global_probing_wraps_past_the_last_slot(lib, panels):
    """16 global slots, 12 keys, of which three have the last slot for a home and two the one before."""
    cp = panels["c1"]
    rng = np.random.default_rng(12)
    b = Batch(cp, 120, rng)
    codes = rng.integers(0, 4, (4000, b.W))
    slot = (hash_np(keys_of_flanks(codes, 1, 1)) & np.uint64(15)).astype(np.int64)
    rows = list(np.flatnonzero(slot == 15)[:3]) + list(np.flatnonzero(slot == 14)[:2]) + list(np.flatnonzero(slot < 13)[:7])
    flanks = [letters(codes[r]) for r in rows]
    assert len(set(flanks)) == 12
    for i in range(len(b.lens)):
        for e in (0, 1):
            b.plant(i, 1, e, flanks[int(rng.integers(12))], 1)
    want, want_counters, _cat, _keys = b.reference()
    homes = sorted(stats_hash(key) & 15 for key in want)
    assert len(want) == 12 and homes.count(15) == 3 and homes.count(14) == 2   # at least three keys wrap to slots 0..
    (got,) = count_on_device(cp, b, 16)
    assert_equal(got, want, want_counters)
    assert sum(got[0].values()) == 240


def stride_batch(cp, n_reads, rng, hits_from=0):
    """Sparse hits from a pool of 200 flanks, on reads hits_from and up."""
    b = Batch(cp, n_reads, rng)
    pool = [letters(rng.integers(0, 4, b.W)) for _ in range(200)]
    for i in np.flatnonzero(rng.integers(0, 16, n_reads) == 0):
        if i >= hits_from:
            b.plant(int(i), int(rng.integers(b.NP)), int(rng.integers(2)), pool[int(rng.integers(200))], int(rng.integers(2)))
    return b


def test_grid_stride_takes_further_steps(lib, panels):
    """The launch is capped at two workgroups per CU: more items than that, with hits only past the first stride -- in the
    second and in the last, partial one -- then exactly one stride of items, and one read more."""
    import torch
    cp = panels["c1"]
    H = 2 * len(cp.primers)
    stride = 2 * torch.cuda.get_device_properties(0).multi_processor_count * LANES     # items of one step of the whole grid
    assert stride % H == 0
    rng = np.random.default_rng(13)
    n_reads = (2 * stride + 5 * LANES + 8) // H
    b = stride_batch(cp, n_reads, rng, hits_from=stride // H)
    want, want_counters, cat, _keys = b.reference()
    flat = cat.reshape(-1)
    assert len(flat) > 2 * stride and len(flat) % stride != 0 and len(flat) % LANES != 0
    assert not flat[:stride].any() and (flat[stride:2 * stride] == COUNTED).sum() > 1000 and (flat[2 * stride:] == COUNTED).sum() >= 20
    (got,) = count_on_device(cp, b, 1 << 12)
    assert_equal(got, want, want_counters)
    for extra in (0, 1):                                                               # one stride exactly, and one read more
        b = stride_batch(cp, stride // H + extra, rng)
        want, want_counters, cat, _keys = b.reference()
        assert cat.size == stride + extra * H
        if extra:
            b.plant(len(b.lens) - 1, 0, 1, "A" * b.W, 1)                               # the read past the stride holds a hit
            want, want_counters, cat, _keys = b.reference()
            assert cat[-1, 1] == COUNTED
        (got,) = count_on_device(cp, b, 1 << 12)
        assert_equal(got, want, want_counters)


def every_category_batch(cp, rng, n=400):
    """Random records of every primer: no hit, pruned, reads shorter than S, primer ends all over the window (flanks from
    0 bases up), windows with N and lower-case letters."""
    b = Batch(cp, n, rng)
    S = b.S
    noise = rng.integers(0, 40, (n, 2 * S))
    b.windows[:, :2 * S][noise == 0] = ord("N")
    b.windows[:, :2 * S][noise == 1] = ord("a")
    b.lens[rng.integers(0, 5, n) == 0] = S - 1
    b.lens[rng.integers(0, 9, n) == 0] = S
    shape = b.hits.shape
    b.hits["pdist"] = np.where(rng.integers(0, 4, shape) == 0, -1, rng.integers(0, 3, shape))
    b.hits["bbest"] = rng.integers(-2, 3, shape)
    j_end = np.where(rng.integers(0, 2, shape) == 0, rng.integers(0, S, shape), S - 1 - rng.integers(0, b.W + 4, shape))
    b.hits["first_end"] = j_end + (b.lens[:, None] - S)
    return b


def test_counters_of_every_primer_in_every_category_and_twice(lib, panels):
    from test_flank_gpu import brute_force
    cp = panels["c3"]
    b = every_category_batch(cp, np.random.default_rng(14))
    want, want_counters, cat, keys = b.reference()
    # the numpy restatement against the suite's brute force, record by record
    table, counters, records = brute_force(cp, b.windows, b.lens, b.hits)
    assert table == want and np.array_equal(counters, want_counters) and len(records) == int((cat > 0).sum())
    for i, p, e, c, key in records:
        assert cat[i, 2 * p + e] == c and (key is None or key == int(keys[i, 2 * p + e]))
    print(want_counters.tolist())
    assert want_counters.shape == (8, 6) and (want_counters[:, [PRUNED, SHORT_READ, SHORT_FLANK, AMBIGUOUS, COUNTED]] >= 10).all()
    assert (want_counters[:, HITS] == want_counters[:, 1:].sum(axis=1)).all()
    flens = {key >> 52 & 31 for key in want}
    assert flens == set(range(b.Lb - b.k, b.W + 1))                      # every flank length a key can hold
    once, again = count_on_device(cp, b, 1 << 14, times=2)
    assert_equal(once, want, want_counters)
    assert_equal(again, want, want_counters)


def test_make_key_is_the_layout_the_kernel_writes(lib, panels):
    """flank_utils.make_key, which the assign tests build their keys with, against the keys the count kernel leaves."""
    cp = panels["c1"]
    rng = np.random.default_rng(15)
    b = Batch(cp, 64, rng)
    planted = {}
    for i in range(64):
        flank, p, e, matched = letters(rng.integers(0, 4, b.W)), int(rng.integers(2)), int(rng.integers(2)), int(rng.integers(2))
        b.plant(i, p, e, flank, matched)
        key = make_key(flank, matched, p)
        planted[key] = planted.get(key, 0) + 1
    (got,) = count_on_device(cp, b, 1 << 10)
    assert got[0] == planted
