"""calls.msa's argument list, byte for byte, against the recording stand-in for the library of test_calls_cpu.py, with
expectations written from include/smx.h: smx_msa(seqs, off, n, merges, mismatch, gap, cap_cols, rows, n_cols, lens, costs,
kernel_ms); and its one retry after SMX_ERR_OVERFLOW.  No GPU and no libsmx.so needed."""
import numpy as np
import pytest

from specimux_amd import _lib, calls
from test_calls_cpu import KEY, MS, WORD, FakeLib, Out, call, fake, same, u64  # noqa: F401

MERGE = np.dtype([("a", "<u4"), ("b", "<u4")])
SEQS = [b"ACGT", b"GG", b"TTTAA"]
BLOB, OFF = b"ACGTGGTTTAA", u64(0, 4, 6, 11)
MERGES = np.array([(2, 0), (3, 1)], dtype=MERGE)


def test_the_record_and_the_limits_are_the_header_s():
    assert _lib.MSA_MERGE_DTYPE == MERGE and MERGE.itemsize == 8
    assert (_lib.MSA_MAX_N, _lib.MSA_MAX_COLS) == (4096, 8192)


def outputs(n, cap, n_cols):
    return (Out("u1", n * cap, 0x5A, fill=np.arange(n * cap) % 251), Out("<u4", 1, WORD, fill=[n_cols]),
            Out("<u4", max(n - 1, 1), WORD), Out("<u8", max(n - 1, 1), KEY))


def test_msa(fake):  # noqa: F811
    rows, n_cols, lens, costs = outputs(3, 2 * 5 + 64, 7)             # the default room: twice the longest and 64
    got = call(fake, "smx_msa", [BLOB, OFF, 3, MERGES, 2, 3, 74, rows, n_cols, lens, costs], calls.msa,
               SEQS, [(2, 0), (3, 1)], 2, 3, None)
    same(got[0], rows.written[:21].reshape(3, 7))                     # n rows of stride n_cols
    same(got[1], lens.written)
    same(got[2], costs.written)


def test_msa_defaults_and_any_pairs(fake):  # noqa: F811
    rows, n_cols, lens, costs = outputs(3, 9, 9)
    fake.layout = [BLOB, OFF, 3, MERGES, 1, 1, 9, rows, n_cols, lens, costs]
    got = calls.msa(SEQS, np.array([[2, 0], [3, 1]], dtype=np.int64), cap_cols=9)
    (name, seen), = fake.log
    assert name == "smx_msa" and seen[3] == MERGES.tobytes() and seen[4:7] == [1, 1, 9]
    assert got[0].shape == (3, 9)


@pytest.mark.parametrize("n", [0, 1])
def test_msa_without_merges(fake, n):  # noqa: F811
    # no null pointer even where the library needs none: one record's room, one entry of lens and costs
    seqs = SEQS[:n]
    rows, n_cols, lens, costs = outputs(n, 2 * 4 * n + 64, 4 * n)
    layout = [b"".join(seqs), OFF[:n + 1], n, np.zeros(1, dtype=MERGE), 1, 1, 8 * n + 64, rows, n_cols, lens, costs]
    rows.count = max(rows.count, 1)
    rows.fill = np.arange(rows.count) % 251
    got = call(fake, "smx_msa", layout, calls.msa, seqs, [], 1, 1, None)
    assert got[0].shape == (n, 4 * n) and got[1].shape == (0,) and got[2].shape == (0,)


def test_msa_refuses_another_number_of_merges(fake):  # noqa: F811
    with pytest.raises(ValueError, match="merges"):
        calls.msa(SEQS, [(0, 1)])
    with pytest.raises(ValueError, match="merges"):
        calls.msa(SEQS[:1], [(0, 1)])
    assert fake.log == []


class Overflowing(FakeLib):
    """Reports SMX_ERR_OVERFLOW and `need` columns while cap_cols is below `need`, then succeeds."""

    def __init__(self, need):
        super().__init__()
        self.need = need

    def _call(self, name, args):
        cap = args[6]
        self.layout = [BLOB, OFF, 3, MERGES, 1, 1, cap, *outputs(3, cap, self.need)]
        super()._call(name, args)
        return _lib.ERR_OVERFLOW if cap < self.need else _lib.OK


def test_one_retry_with_the_reported_columns(monkeypatch):
    lib = Overflowing(need=80)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    ms = []
    rows, lens, costs = calls.msa(SEQS, [(2, 0), (3, 1)], kernel_ms=ms)
    assert [seen[6] for _, seen in lib.log] == [74, 80] and ms == [MS, MS]
    assert rows.shape == (3, 80)
    assert all(seen[7] == bytes([0x5A]) * (3 * seen[6]) for _, seen in lib.log)     # fresh sentinel-filled rows each time


def test_no_second_retry(monkeypatch):
    class Stubborn(Overflowing):
        def _call(self, name, args):
            super()._call(name, args)
            return _lib.ERR_OVERFLOW
    lib = Stubborn(need=80)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    ms = []
    with pytest.raises(_lib.SmxError, match="refused by the fake") as err:
        calls.msa(SEQS, [(2, 0), (3, 1)], kernel_ms=ms)
    assert err.value.code == _lib.ERR_OVERFLOW and len(lib.log) == 2 and ms == []


def test_status(monkeypatch):
    """A nonzero status raises SmxError with the library's message; no device time is handed over."""
    lib = FakeLib(status=_lib.ERR_ARG)
    lib.layout = [BLOB, OFF, 3, MERGES, 1, 1, 74, *outputs(3, 74, 7)]
    monkeypatch.setattr(_lib, "load", lambda: lib)
    ms = []
    with pytest.raises(_lib.SmxError, match="refused by the fake") as err:
        calls.msa(SEQS, [(2, 0), (3, 1)], kernel_ms=ms)
    assert err.value.code == _lib.ERR_ARG and ms == [] and len(lib.log) == 1
