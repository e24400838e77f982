"""stats_kernel (specimux_amd/csrc/smx_stats.hip) on synthetic hit tables, through smx_stats_accumulate_device: hit records
and primary records are built in numpy (tests/stats_utils.py case_*) and uploaded with torch, the panel only supplies NP, the
primer directions and the pair list.  Every table is compared with == against stats_utils.rows_reference, a restatement of
the row rule from its definition that tests/test_stats_cpu.py checks against the CPU simulation on these same inputs; there
`local_spill` also counts the rows that pass the workgroup's table by, which the kernel cannot report.  Here each test
asserts by arithmetic on its inputs that its edge is reached: the truth table of hit states (A), random hits (B), more keys
on one LDS home slot than a probe run holds, at the table's last slot (C), a global table exactly full and one key too many
(D), a grid stride with a remainder (E), the fallback list and its cap (F), the key fields at their largest values (G)."""
import ctypes as C

import numpy as np
import pytest

import stats_utils as U
from parity_utils import Both, tmp_panel

pytestmark = pytest.mark.gpu
SENTINEL = 0x5EED5EED                       # prefill of every buffer the library writes
KEY_SENTINEL = np.uint64(0x5EED5EED5EED5EED)


@pytest.fixture(scope="module")
def lib():
    from specimux_amd import _lib
    lib = _lib.load()
    n = C.c_int(0)
    _lib.check(lib.smx_device_init(0, C.byref(n)))
    assert n.value >= 1
    return lib


@pytest.fixture(scope="module")
def panels(lib, tmp_path_factory):
    """{(c2 | c3 | c9, preorient): (compiled panel, NP, pdir, pairs)}, c9 = stats_utils.panel_nine_pairs: the panel facts come
    from the oracle's view of the panel and are asserted equal to the product's."""
    from specimux_amd import synth
    from specimux_amd.demultiplex import compiled_panel
    out = {}
    for name, pan in (("c2", synth.panel_c2()), ("c3", synth.panel_c3()), ("c9", U.panel_nine_pairs())):
        pf, sf = tmp_panel(tmp_path_factory, pan, "stats_kernel_" + name)
        for preorient in (True, False):
            both = Both(pf, sf, disable_preorient=not preorient)
            cp = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
            view = U.panel_view(both.opanel)
            NP = len(view.primers)
            assert view.primer_names == cp.primer_names and view.pairs == [tuple(p) for p in cp.pairs]
            assert cp.hits_per_read == 2 * NP and bool(cp.desc.preorient) == preorient
            out[name, preorient] = (cp, NP, view.pdir, view.pairs)
            out[name, "barcodes"] = len(view.barcodes)
    assert out["c2", True][1] == 2 and out["c3", True][1] == out["c9", True][1] == 8
    assert len(out["c3", True][3]) == 4 and len(out["c9", True][3]) == 9
    return out


def reference(panel, preorient, hits, ops):
    _cp, NP, pdir, pairs = panel
    return U.rows_reference(NP, pdir, pairs, preorient, hits, ops)


class Device:
    """One statistics table and the device copies of one case's records."""

    def __init__(self, lib, cp, capacity, hits, ops):
        import torch
        from specimux_amd import _lib, trace_stats
        assert hits.dtype == U.HIT == _lib.HIT_DTYPE and ops.dtype == U.OP == _lib.OP_DTYPE and hits.shape == (len(ops), cp.hits_per_read)
        self.torch, self.lib, self.n = torch, lib, len(ops)
        self.d_hits = torch.from_numpy(np.ascontiguousarray(hits).view(np.uint8).reshape(-1).copy()).cuda()
        self.d_ops = torch.from_numpy(np.ascontiguousarray(ops).view(np.uint8).reshape(-1).copy()).cuda()
        self.slots = 8
        while self.slots < capacity:
            self.slots *= 2
        self.stats = trace_stats.DeviceStats(cp, capacity)
        torch.cuda.synchronize()

    def records(self, hits, ops):
        """Other records for the same table."""
        self.n = len(ops)
        self.d_hits = self.torch.from_numpy(np.ascontiguousarray(hits).view(np.uint8).reshape(-1).copy()).cuda()
        self.d_ops = self.torch.from_numpy(np.ascontiguousarray(ops).view(np.uint8).reshape(-1).copy()).cuda()
        self.torch.cuda.synchronize()

    def accumulate(self, fallback_cap=None, with_list=True, null_list=False):
        """One smx_stats_accumulate_device -> (*d_n_fallback, the whole fallback buffer), both prefilled with SENTINEL; or
        (None, None) for the call without a list and without a counter.  null_list: d_fallback = NULL with cap 0, the
        counter stays."""
        torch = self.torch
        if not with_list:
            self.stats.accumulate(None, self.d_hits.data_ptr(), self.d_ops.data_ptr(), self.n, None, 0, None)
            torch.cuda.synchronize()
            return None, None
        d_list = torch.full((self.n + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        d_n = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.stats.accumulate(None, self.d_hits.data_ptr(), self.d_ops.data_ptr(), self.n, None if null_list else d_list.data_ptr(),
                              0 if null_list else self.n if fallback_cap is None else fallback_cap, d_n.data_ptr())
        torch.cuda.synchronize()
        d_n, d_list = d_n.cpu().numpy(), d_list.cpu().numpy()
        assert d_n[1:].tolist() == [SENTINEL] * 3                # one word is written
        assert not null_list or (d_list == SENTINEL).all()
        return int(d_n[0]), d_list

    def read_raw(self):
        """smx_stats_read into prefilled buffers -> (status, *n, *dropped, keys, counts)."""
        from specimux_amd import _lib
        keys, counts = np.full(self.slots + 1, KEY_SENTINEL), np.full(self.slots + 1, KEY_SENTINEL)
        n, dropped = C.c_uint32(SENTINEL), C.c_uint64(SENTINEL)
        rc = self.lib.smx_stats_read(self.stats.handle, _lib.ptr(keys), _lib.ptr(counts), self.slots, C.byref(n), C.byref(dropped))
        return rc, n.value, dropped.value, keys, counts

    def read(self):
        """{key: count}; nothing lost, one slot per key, nothing written past the keys."""
        rc, n, dropped, keys, counts = self.read_raw()
        assert rc == 0 and dropped == 0 and n <= self.slots
        assert (keys[n:] == KEY_SENTINEL).all() and (counts[n:] == KEY_SENTINEL).all()
        assert len(set(keys[:n].tolist())) == n
        return dict(zip(keys[:n].tolist(), counts[:n].tolist()))

    def close(self):
        self.stats.close()


def assert_table(got, want, label=""):
    want = dict(want)
    assert got == want, (label, len(got), len(want), [(hex(k), got.get(k), want.get(k)) for k in set(got) | set(want)
                                                       if got.get(k) != want.get(k)][:6])


def assert_list(n_fallback, buf, want, cap=None):
    """The fallback counter is the reference's count; the buffer holds min(count, cap) distinct reads of the reference's
    list and the prefill behind them."""
    cap = len(want) if cap is None else cap
    stored = min(cap, len(want))
    assert n_fallback == len(want)
    got = buf[:stored].tolist()
    assert len(set(got)) == stored and set(got) <= set(want)
    if cap >= len(want):
        assert sorted(got) == want
    assert (buf[stored:] == SENTINEL).all()


def count(lib, panel, hits, ops, capacity, want, label=""):
    """One call over one case on a fresh table: table and fallback list against `want` = (table, fallback list)."""
    dev = Device(lib, panel[0], capacity, hits, ops)
    try:
        n_fallback, buf = dev.accumulate()
        assert_table(dev.read(), want[0], label)
        assert_list(n_fallback, buf, want[1])
    finally:
        dev.close()


# ------------------------------------------------------------------ A: the truth table of hit states
@pytest.fixture(scope="module")
def truth_table():
    return U.case_truth_table()


@pytest.mark.parametrize("preorient", [True, False])
def test_truth_table_of_hit_states(lib, panels, truth_table, preorient):
    """12 states per hit record (primer found or not, barcode pruned / not found / found, vote bit) on all four records of a
    two-primer panel = 20 736 hit rows, each with every rtype 0..6 and the record flags cycling with period 5: barcode hits
    without a primer hit, votes without a primer hit, every class against every candidate shape."""
    hits, ops = truth_table
    panel = panels["c2", preorient]
    want = reference(panel, preorient, hits, ops)
    assert len(ops) == 12 ** 4 * 7
    assert {(r, f) for r, f in zip(ops["rtype"].tolist(), ops["flags"].tolist())} == {(r, f) for r in range(7) for f in U._OP_FLAGS}
    U.assert_truth_table_coverage(want[0], want[1], ops, preorient)
    count(lib, panel, hits, ops, 1 << 10, want, f"preorient {preorient}")


# ------------------------------------------------------------------ B: random hits on eight primers
@pytest.fixture(scope="module")
def random_case(panels):
    """(hits, ops, {preorient: rows of every read}) of case B."""
    _cp, NP, pdir, pairs = panels["c9", True]
    hits, ops = U.case_random(NP, panels["c9", "barcodes"] - 1)
    return hits, ops, {pre: U.rows_per_read(NP, pdir, pairs, pre, hits, ops) for pre in (True, False)}


@pytest.mark.parametrize("preorient", [True, False])
def test_random_hits_on_eight_primers(lib, panels, random_case, preorient):
    """20 000 reads with random states on all 16 hit records, barcode indices from {0, 1, the panel's last, 8 189}, on the
    eight primers of c3 in nine pairs (c3's own four pairs have at most 1 681 keys to give without an orientation): several
    candidates per read, most of them discarded, and with either preorient setting more distinct keys than a workgroup's
    table has slots.  A workgroup of this launch counts 256 reads, though, so here the case pins the rows and their
    counting under many keys; that rows pass a workgroup's table by is case C's to prove on the device, and on these
    inputs the CPU simulation's `local_spill` with one workgroup and with seven (tests/test_stats_cpu.py)."""
    hits, ops, rows = random_case
    panel = panels["c9", preorient]
    want = reference(panel, preorient, hits, ops)
    assert len(ops) == 20000 and len(want[0]) >= U.LCAP + 1 == 2049
    assert want[0] == U.reference_of_templates(rows[preorient], np.arange(len(ops)), np.arange(len(ops)))[0]
    fields = [U.fields_of(key) for key in want[0]]
    assert {f[4] for f in fields} == {f[5] for f in fields} == {0, 1, 2, panels["c9", "barcodes"], 8190}
    assert {f[1] for f in fields} == set(range(len(panel[3]) + 1)) and {f[6] for f in fields} == set(range(6))
    assert sum(c for key, c in want[0].items() if key >> 42 & 7 == U.CLASS_DISCARDED) >= 20000
    count(lib, panel, hits, ops, 1 << 13, want, f"preorient {preorient}")


# ------------------------------------------------------------------ C: LDS bypass, LDS wrap, global wrap
@pytest.mark.parametrize("uses", list(U.BYPASS_USES))
def test_keys_of_the_last_lds_slot_bypass_and_wrap(lib, panels, uses):
    """40 one-row keys whose home in the workgroup's table is its last slot, 2 047: every probe run wraps to slot 0, and a
    workgroup that meets more than STATS_LPROBE of them sends the rest to the global table directly, whichever lanes win
    the claims.  The global table has 64 slots: all 40 start at its last slot and wrap too.  "1+j%6": 136 reads, one
    workgroup, key j 1 + j % 6 times -- at least 24 keys bypass.  "8x256" and "48x256": the same keys 51 or 52 and 300 to
    314 times each over 8 and 48 workgroups, whose flushed counts and direct adds meet on the same global slots."""
    panel = panels["c3", True]
    _cp, NP, pdir, pairs = panel
    hits, ops, _b = U.case_bypass(NP, pairs[0], 1, U.BYPASS_USES[uses], 71)
    rows = U.rows_per_read(NP, pdir, pairs, True, hits, ops)
    want = reference(panel, True, hits, ops)
    assert all(r is not None and len(r) == 1 for r in rows) and len(want[0]) == 40 and want[1] == []
    home = U.stats_hash_np(np.array(list(want[0]), dtype=np.uint64))
    assert set((home & np.uint64(U.LCAP - 1)).tolist()) == {U.LCAP - 1} and set((home & np.uint64(63)).tolist()) == {63}
    assert U.LPROBE == 16 and 40 - U.LPROBE >= 24
    if uses == "1+j%6":
        assert len(ops) <= U.THREADS and sorted(want[0].values()) == sorted((1 + np.arange(40) % 6).tolist())
    else:
        groups = len(ops) // U.THREADS
        assert len(ops) == groups * U.THREADS and groups == int(uses.split("x")[0])
        # every workgroup meets more of the keys than a probe run holds
        seen = [len({r[0] for r in rows[g * U.THREADS:(g + 1) * U.THREADS]}) for g in range(groups)]
        assert min(seen) > U.LPROBE + 8 and min(want[0].values()) >= (300 if groups == 48 else 51)
    count(lib, panel, hits, ops, 64, want, uses)


# ------------------------------------------------------------------ D: the global table exactly full, then one key too many
def test_global_table_exactly_full_then_one_key_too_many(lib, panels):
    """Eight slots, the smallest table.  D1: eight keys with the last slot for a home, five times each, fill it exactly.
    D2, after smx_stats_clear: nine such keys.  Slots are never released and every probe run covers the whole table, so
    exactly one key finds no slot, and with five uses of every key five increments are lost whichever key it is:
    smx_stats_read fails with SMX_ERR_OVERFLOW, *n = 0, *dropped = 5 and copies nothing.  D3, after another clear: D1's
    result again."""
    from specimux_amd import _lib
    panel = panels["c3", True]
    _cp, NP, pdir, pairs = panel
    eight, nine = U.case_full_table(NP, pairs[0], 1, 8), U.case_full_table(NP, pairs[0], 1, 9)
    want8, want9 = reference(panel, True, *eight), reference(panel, True, *nine)
    assert sorted(want8[0].values()) == [5] * 8 and sorted(want9[0].values()) == [5] * 9 and len(nine[1]) == 45 <= U.THREADS
    assert set(want8[0]) < set(want9[0])
    assert set((U.stats_hash_np(np.array(list(want9[0]), dtype=np.uint64)) & np.uint64(7)).tolist()) == {7}
    dev = Device(lib, panel[0], 8, *eight)
    try:
        assert dev.slots == 8
        for step in ("D1", "D2", "D3"):
            dev.records(*(nine if step == "D2" else eight))
            n_fallback, _buf = dev.accumulate()
            assert n_fallback == 0
            if step == "D2":
                rc, n, dropped, keys, counts = dev.read_raw()
                assert (rc, n, dropped) == (_lib.ERR_OVERFLOW, 0, 5), (rc, n, dropped)
                assert (keys == KEY_SENTINEL).all() and (counts == KEY_SENTINEL).all()
                assert "8 slots" in lib.smx_last_error().decode() and "5 increments" in lib.smx_last_error().decode()
            else:
                assert_table(dev.read(), want8[0], step)
            dev.stats.clear()
    finally:
        dev.close()


# ------------------------------------------------------------------ E: the grid-stride loop with a remainder
def test_grid_stride_with_a_remainder(lib, panels, random_case, monkeypatch):
    """One workgroup per CU (SMX_STATS_BLOCKS_PER_CU=1) and 2 G 256 + 77 reads for G CUs: every thread takes a second read,
    77 threads of the first workgroup a third.  The reads are drawn from 500 (hit row, record) templates of case B, each
    also used past the grid's first step; the 77 reads of the last, partial step use 77 different templates that give
    rows (500 templates cannot all fall on 77 reads).  The reference takes each template's rows once, times its uses."""
    import torch
    monkeypatch.setenv("SMX_STATS_BLOCKS_PER_CU", "1")
    G = torch.cuda.get_device_properties(0).multi_processor_count
    hits_b, ops_b, rows_b = random_case
    hits, ops, use, pool = U.case_stride(hits_b, ops_b, rows_b[True], G)
    n, step = len(ops), G * U.THREADS
    assert n == 2 * step + 77 and n > step and n % step == 77 and len(pool) == len(set(pool.tolist())) == 500
    assert set(use[step:].tolist()) == set(range(500))                   # every template past the first step
    tail = use[2 * step:].tolist()
    assert len(tail) == len(set(tail)) == 77 and all(rows_b[True][pool[t]] for t in tail)
    want = U.reference_of_templates(rows_b[True], pool, use)
    assert sum(want[0].values()) > n and len(want[1]) > 100
    count(lib, panels["c9", True], hits, ops, 1 << 13, want)


# ------------------------------------------------------------------ F: the fallback list
def test_fallback_list_cap_and_null_arguments(lib, panels):
    """3 000 reads of case A's kind, about 700 of them unfiltered with SMX_OPF_TRIM_EMPTY.  (i) a list as long as the batch;
    (ii) a list of 100: the counter still says how many there are, 100 distinct ones are stored, the buffer behind them is
    untouched; (iii) no list and no counter, and no list with a counter; (iv) two calls into one table count everything
    twice.  The table never
    holds a row of a listed read: it equals the reference's, which gives them none."""
    panel = panels["c2", True]
    hits, ops = U.case_fallback()
    want = reference(panel, True, hits, ops)
    k = len(want[1])
    flagged = (ops["flags"] & U.OPF_TRIM_EMPTY) != 0
    assert len(ops) == 3000 and 600 <= k <= 800 and k == int((flagged & (ops["rtype"] != U.R_FILTERED)).sum()) < int(flagged.sum())
    assert sum(c for key, c in want[0].items() if key & U.FIRST) == 3000 - k
    dev = Device(lib, panel[0], 1 << 10, hits, ops)
    try:
        for cap in (len(ops), 100):                                      # (i), (ii)
            n_fallback, buf = dev.accumulate(fallback_cap=cap)
            assert_list(n_fallback, buf, want[1], cap)
            assert_table(dev.read(), want[0], f"cap {cap}")
            dev.stats.clear()
        dev.accumulate(with_list=False)                                  # (iii)
        assert_table(dev.read(), want[0], "no list")
        n_fallback, buf = dev.accumulate(fallback_cap=0)                 # (iv), and a list of no entries
        assert_list(n_fallback, buf, want[1], 0)
        assert_table(dev.read(), {key: 2 * c for key, c in want[0].items()}, "two calls")
        dev.stats.clear()
        assert dev.accumulate(null_list=True)[0] == k                    # d_fallback = NULL beside a real counter
        assert_table(dev.read(), want[0], "a counter without a list")
    finally:
        dev.close()


# ------------------------------------------------------------------ G: the key fields at their edges
def test_key_fields_at_their_edges(lib, panels):
    """The largest barcode field smx_stats_create admits (8 190, first_tied = 8 189) at either end and at both, beside an
    empty field, on every pair up to the last (pair field = NPAIR) and with every rtype 1..6."""
    panel = panels["c3", True]
    _cp, NP, pdir, pairs = panel
    hits, ops = U.case_field_edges(NP, pairs)
    want = reference(panel, True, hits, ops)
    assert int(hits["first_tied"].max()) == 8189 and len(ops) == 18 * len(pairs)
    U.assert_field_edges(want[0], len(pairs))
    dev = Device(lib, panel[0], 1 << 8, hits, ops)
    try:
        assert dev.accumulate()[0] == 0
        got = dev.read()
    finally:
        dev.close()
    for key, c in got.items():                                           # decoded here, bit by bit
        assert key >> 46 == 0 and key & 3 == 1 and key >> 14 & 3 == 3 and key >> 45 & 1 == 1
        assert 1 <= (key >> 2 & 0xfff) <= len(pairs) and (key >> 16 & 0x1fff, key >> 29 & 0x1fff) in ((8190, 8190), (8190, 0), (0, 8190))
        assert (key >> 42 & 7, c) in ((0, 2), (1, 1), (2, 1), (3, 1), (4, 1))
    assert sum(1 for key in got if key >> 2 & 0xfff == len(pairs)) == 15
    assert_table(got, want[0])
