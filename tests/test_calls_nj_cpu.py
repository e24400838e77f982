"""calls.nj's argument list, byte for byte, against the recording stand-in for the library of test_calls_cpu.py, with
expectations written from include/smx.h: smx_nj(tri, n, merges, last, last_d, kernel_ms).  No GPU and no libsmx.so
needed."""
import numpy as np
import pytest

from specimux_amd import _lib, calls
from test_calls_cpu import KEY, WORD, FakeLib, Out, call, fake, i32, same  # noqa: F401

MERGE = np.dtype([("a", "<u4"), ("b", "<u4"), ("n_active", "<u4"), ("pad", "<u4"), ("d", "<f8"), ("ra", "<f8"), ("rb", "<f8")])


def test_the_record_is_the_header_s():
    assert _lib.NJ_MERGE_DTYPE == MERGE and MERGE.itemsize == 40
    assert [MERGE.fields[f][1] for f in MERGE.names] == [0, 4, 8, 12, 16, 24, 32]


def test_nj(fake):  # noqa: F811
    tri = i32(3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9)          # n = 6
    merges, last, last_d = Out("<u8", 15, KEY), Out("<u4", 3, WORD), Out("<u8", 3, KEY)   # 3 records of 40 bytes
    got = call(fake, "smx_nj", [tri, 6, merges, last, last_d], calls.nj, tri, 6)
    assert len(got) == 3
    same(got[0], merges.written.view(MERGE), (3,))
    same(got[1], last.written)
    same(got[2], last_d.written.view("<f8"))


def test_nj_takes_any_integer_sequence(fake):  # noqa: F811
    merges, last, last_d = Out("<u8", 5, KEY), Out("<u4", 3, WORD), Out("<u8", 3, KEY)
    got = call(fake, "smx_nj", [i32(1, 2, 3, 4, 5, 6), 4, merges, last, last_d], calls.nj, [1, 2, 3, 4, 5, 6], np.int64(4))
    assert got[0].shape == (1,) and got[0].dtype == MERGE


@pytest.mark.parametrize("n, tri", [(0, []), (1, []), (2, [7]), (3, [7, 8, 9])])
def test_nj_without_merges(fake, n, tri):  # noqa: F811
    # no null pointer even where the library needs none: one record's room, one zero for an empty triangle
    layout = [i32(*tri) if tri else i32(0), n, Out("<u8", 5, KEY), Out("<u4", 3, WORD), Out("<u8", 3, KEY)]
    got = call(fake, "smx_nj", layout, calls.nj, tri, n)
    assert got[0].shape == (0,) and got[0].dtype == MERGE and got[1].shape == (3,) and got[2].shape == (3,)


@pytest.mark.parametrize("n, tri", [(4, [1, 2, 3]), (3, [1, 2, 3, 4]), (-1, []), (2, [])])
def test_nj_refuses_a_triangle_of_another_size(fake, n, tri):  # noqa: F811
    with pytest.raises(ValueError, match="tri"):
        calls.nj(tri, n)
    assert fake.log == []


def test_status(monkeypatch):
    """A nonzero status raises SmxError with the library's message; no device time is handed over."""
    lib = FakeLib(status=_lib.ERR_ARG)
    lib.layout = [i32(7), 2, Out("<u8", 5, KEY), Out("<u4", 3, WORD), Out("<u8", 3, KEY)]
    monkeypatch.setattr(_lib, "load", lambda: lib)
    ms = []
    with pytest.raises(_lib.SmxError, match="refused by the fake") as err:
        calls.nj([7], 2, ms)
    assert err.value.code == _lib.ERR_ARG and ms == []
