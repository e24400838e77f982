"""calls.cons_profile's argument list, byte for byte, against the recording stand-in for the library of test_calls_cpu.py,
with expectations written from include/smx.h: smx_cons_profile(reads, roff, n_reads, k, jobs, n_jobs, quals, votes,
aligned, per_member, tables, kernel_ms).  No GPU and no libsmx.so needed."""
import pytest

from specimux_amd import _lib, calls
from test_calls_cpu import CONS_EMPTY, CONS_HEAD, CONS_JOBS, KS, S, WORD, FakeLib, Out, call, fake, same  # noqa: F401

QUALS = [b"IIII", b"", b"!~", b"5555+", b"#"]               # one string per sequence of S, of its length


def test_cons_profile(fake):  # noqa: F811
    votes, aligned = Out("<u4", 312, 0), Out("<u4", 3, 0)          # (5 + 6 + 1) rows of 26 words
    members, tables = Out("<u4", 40, WORD), Out("<u4", 822, WORD)  # (2 + 0 + 3) members x 8 words; 3 jobs x 274 words
    layout = CONS_HEAD + [b"IIII!~5555+#", votes, aligned, members, tables]
    got = call(fake, "smx_cons_profile", layout, calls.cons_profile, S, QUALS, KS, CONS_JOBS)
    assert len(got) == 3 and all(len(job) == 4 for job in got)
    for j, (lo, hi, rows) in enumerate(((0, 130, 5), (130, 286, 6), (286, 312, 1))):
        same(got[j][0], votes.written[lo:hi], (rows, 26))
        assert got[j][1] == int(aligned.written[j]) and type(got[j][1]) is int
        same(got[j][3], tables.written[274 * j:274 * j + 274])
    same(got[0][2], members.written[0:16], (2, 8))
    assert got[1][2].shape == (0, 8)
    same(got[2][2], members.written[16:40], (3, 8))


def test_cons_profile_empty(fake):  # noqa: F811
    layout = CONS_EMPTY + [b"", Out("<u4", 1, 0), Out("<u4", 1, 0), Out("<u4", 1, WORD), Out("<u4", 1, WORD)]
    assert call(fake, "smx_cons_profile", layout, calls.cons_profile, [], [], [], []) == []


@pytest.mark.parametrize("quals", [QUALS[:4], [b"III"] + QUALS[1:], QUALS + [b""]])
def test_cons_profile_refuses_quality_strings_of_another_shape(fake, quals):  # noqa: F811
    with pytest.raises(ValueError, match="quals"):
        calls.cons_profile(S, quals, KS, CONS_JOBS)
    assert fake.log == []


def test_status(monkeypatch):
    """A nonzero status raises SmxError with the library's message; no device time is handed over."""
    lib = FakeLib(status=_lib.ERR_UNSUPPORTED)
    lib.layout = CONS_EMPTY + [b"", Out("<u4", 1, 0), Out("<u4", 1, 0), Out("<u4", 1, WORD), Out("<u4", 1, WORD)]
    monkeypatch.setattr(_lib, "load", lambda: lib)
    ms = []
    with pytest.raises(_lib.SmxError, match="refused by the fake") as err:
        calls.cons_profile([], [], [], [], ms)
    assert err.value.code == _lib.ERR_UNSUPPORTED and ms == []
