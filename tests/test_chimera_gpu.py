"""specimux-chimera end to end on the reference's golden reads (tests/golden/integration_test_suite): the flags against
this file's own DP (tests/inner_utils.py) plus its own junction rule, the three concatemers the golden file holds, the
clean / flagged split, the reverse-complemented file, 39 artificial concatemers, gzip input, -n and determinism."""
import gzip
import os

import numpy as np
import pytest

from conftest import GOLDEN
from inner_utils import expected
from specimux_amd import chimera

pytestmark = pytest.mark.gpu

PANEL = [f"{GOLDEN}/primers.fasta", f"{GOLDEN}/specimens.txt"]
K, GAP, MARGIN, H = 3, 100, 80, 4


def read_fastq(path):
    """(id, sequence, quality) per record."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt") as fh:
        lines = fh.read().split("\n")
    return [(lines[i][1:].split()[0], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4)]


def raw_records(path):
    """The file's 4-line records as bytes, header line and all."""
    with open(path, "rb") as fh:
        lines = fh.read().split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]


def revcomp(s):
    return s.translate(str.maketrans("ACGTMRWSYKVHDBN", "TGCAKYWSRMBDHVN"))[::-1]


@pytest.fixture(scope="module")
def patterns():
    """(name, strand, sequence) from primers.fasta itself; the tool's own list must hold the same patterns."""
    out = []
    with open(PANEL[0]) as fh:
        lines = [ln.strip() for ln in fh if ln.strip()]
    for head, seq in zip(lines[0::2], lines[1::2]):
        name = head[1:].split()[0]
        out += [(name, "+", seq.upper()), (name, "-", revcomp(seq.upper()))]
    args = chimera.parse_args([*PANEL, "unused.fastq"])
    info = chimera.panel_patterns(*chimera.load_panel(args), K)
    assert sorted(out) == sorted((p.name, p.strand, p.seq) for p in info) and {p.k for p in info} == {K}
    return out


def own_flags(patterns, records):
    """The DP's hits and this file's junction rule: (reads with a hit, flagged reads), as index sets."""
    seqs = [p[2] for p in patterns]
    nhit, _, end = expected(seqs, [K] * len(seqs), [r[1].encode() for r in records], MARGIN, H)
    with_hits, flagged = set(), set()
    for r in range(len(records)):
        if nhit[r].any():
            with_hits.add(r)
        closes = [end[r, j, h] + 1 for j, p in enumerate(patterns) if p[1] == "-" for h in range(min(nhit[r, j], H))]
        opens = [end[r, j, h] - len(p[2]) + 1 for j, p in enumerate(patterns) if p[1] == "+" for h in range(min(nhit[r, j], H))]
        if any(-K <= o - c <= GAP for o in opens for c in closes):
            flagged.add(r)
    return with_hits, flagged


def run_tool(tmp_path, sequence_file, *extra, tag="a"):
    report = tmp_path / f"report_{tag}.tsv"
    assert chimera.main([*PANEL, str(sequence_file), "--report", str(report), *extra]) == 0
    with open(report) as fh:
        text = fh.read()
    lines = text.split("\n")
    assert lines[0] + "\n" == chimera.REPORT_HEADER and lines[-1] == ""
    rows = [ln.split("\t") for ln in lines[1:-1]]
    return text, rows


def flags_of(rows, records):
    index = {rec[0]: i for i, rec in enumerate(records)}
    assert len(index) == len(records)
    with_hits = {index[row[0]] for row in rows}
    flagged = {index[row[0]] for row in rows if row[6] == "1"}
    assert all(row[6] in "01" and (row[6] == "1") == (index[row[0]] in flagged) for row in rows)
    return with_hits, flagged


def test_golden_reads(tmp_path, patterns):
    src = f"{GOLDEN}/sequences.fastq"
    records = read_fastq(src)
    assert len(records) == 40
    clean, flagged_path = tmp_path / "clean.fastq", tmp_path / "flagged.fastq"
    text, rows = run_tool(tmp_path, src, "--clean", str(clean), "--flagged", str(flagged_path))
    with_hits, flagged = flags_of(rows, records)
    assert (with_hits, flagged) == own_flags(patterns, records)
    # the constants of the CPU run behind the feature: three concatemers, twelve reads with any internal hit
    assert flagged == {2, 15, 29} and len(with_hits) == 12
    for row in rows:
        assert int(row[1]) == len(records[[r[0] for r in records].index(row[0])][1]) and 0 <= int(row[4]) <= K
        assert MARGIN <= int(row[5]) < int(row[1]) - MARGIN
    # the split files hold the input's records byte for byte, whole header lines included, in input order
    raw = raw_records(src)
    assert len(raw) == 40 and all(len(rec.split(b"\n")[0].split()) > 1 for rec in raw)     # every golden header has a description
    got_clean, got_flagged = raw_records(clean), raw_records(flagged_path)
    assert len(got_clean) == 37 and len(got_flagged) == 3
    assert got_flagged == [raw[i] for i in (2, 15, 29)]
    assert got_clean == [rec for i, rec in enumerate(raw) if i not in flagged]
    # the same run again: the same bytes
    text2, _ = run_tool(tmp_path, src, tag="b")
    assert text2 == text


def test_reverse_complemented_file(tmp_path, patterns):
    src = f"{GOLDEN}/sequences_rc.fastq"
    records = read_fastq(src)
    _, rows = run_tool(tmp_path, src)
    assert flags_of(rows, records) == own_flags(patterns, records)


def test_artificial_concatemers(tmp_path, patterns):
    """read[i] + read[i + 1]: compared with the DP only.  Most are flagged, but a pair whose joined ends hold no primer
    within 3 edits is not, so a fixed count would pin the fixture and not the code."""
    base = read_fastq(f"{GOLDEN}/sequences.fastq")
    records = [(f"cat{i}", base[i][1] + base[i + 1][1], base[i][2] + base[i + 1][2]) for i in range(39)]
    path = tmp_path / "cat.fastq"
    with open(path, "w") as fh:
        for rid, seq, qual in records:
            fh.write(f"@{rid}\n{seq}\n+\n{qual}\n")
    _, rows = run_tool(tmp_path, path)
    got = flags_of(rows, records)
    assert got == own_flags(patterns, records)
    assert len(got[1]) >= 10


def test_gzip_input_and_num_seqs(tmp_path, patterns):
    records = read_fastq(f"{GOLDEN}/sequences.fastq")
    gz = tmp_path / "sequences.fastq.gz"
    with open(f"{GOLDEN}/sequences.fastq", "rb") as src, gzip.open(gz, "wb") as dst:
        dst.write(src.read())
    _, rows = run_tool(tmp_path, gz)
    assert flags_of(rows, records) == own_flags(patterns, records)
    _, rows10 = run_tool(tmp_path, gz, "-n", "10", tag="n10")
    assert flags_of(rows10, records[:10]) == own_flags(patterns, records[:10])
    args = chimera.parse_args([*PANEL, str(gz), "-n", "10"])
    total, with_hits, n_flagged, per_pattern = chimera.run(args)
    assert total == 10 and n_flagged == 1 and with_hits == len({r[0] for r in rows10})
    assert sum(c for _, c in per_pattern) >= len(rows10)   # the counts include hits beyond the stored H
