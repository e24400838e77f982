"""specimux-chimera without a GPU: the flag rules on hand-made hit arrays (both ends of the junction interval, strand
order, a lone nested hit), the report byte for byte, the panel's patterns, the option parsing and the native clean /
flagged split (host code: whole header lines, FASTA, gzip input, bytes above 0x7f)."""
import argparse
import gzip
import os

import numpy as np
import pytest

from specimux_amd import chimera
from specimux_amd.chimera import PatternInfo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "integration_test_suite")

# two primers, as written and reverse-complemented: patterns 0 / 2 are `+`, 1 / 3 are `-`
INFO = [PatternInfo("P1", "+", "ACGTACGTACGTACGTACGT", 3), PatternInfo("P1", "-", "ACGTACGTACGTACGTACGT", 3),
        PatternInfo("P2", "+", "TTGACCATGACCATGACCATGA", 2), PatternInfo("P2", "-", "TCATGGTCATGGTCATGGTCAA", 2)]
H = 2


def hits(*reads):
    """reads: lists of (pattern, distance, end) in column order per pattern."""
    n = len(reads)
    nhit = np.zeros((n, 4), dtype=np.uint8)
    dist = np.full((n, 4, H), -1, dtype=np.int8)
    end = np.zeros((n, 4, H), dtype=np.int32)
    for r, lst in enumerate(reads):
        for j, d, e in lst:
            h = int(nhit[r, j])
            if h < H:
                dist[r, j, h], end[r, j, h] = d, e
            nhit[r, j] += 1
    return nhit, dist, end


def junction(minus_end, plus_pattern, delta, gap=100):
    """One `-` hit of P1 ending at minus_end and one `+` hit whose nominal start is minus_end + 1 + delta."""
    p = INFO[plus_pattern]
    return hits([(1, 0, minus_end), (plus_pattern, 1, minus_end + 1 + delta + len(p.seq) - 1)])


@pytest.mark.parametrize("plus_pattern", [0, 2])
def test_junction_interval_ends(plus_pattern):
    k = INFO[plus_pattern].k
    for delta, want in ((-k - 1, False), (-k, True), (0, True), (100, True), (101, False)):
        got = chimera.flag_reads(*junction(300, plus_pattern, delta), INFO, "junction", 100)
        assert got.tolist() == [want], (plus_pattern, delta)
    assert chimera.flag_reads(*junction(300, plus_pattern, 7), INFO, "junction", 6).tolist() == [False]
    assert chimera.flag_reads(*junction(300, plus_pattern, 6), INFO, "junction", 6).tolist() == [True]


def test_plus_before_minus_is_no_junction():
    # an opening primer at 200-219 and a closing one ending at 600: one whole amplicon, nested, not a junction
    arrays = hits([(0, 0, 219), (3, 0, 600)])
    assert chimera.flag_reads(*arrays, INFO, "junction", 100).tolist() == [False]
    assert chimera.flag_reads(*arrays, INFO, "any", 100).tolist() == [True]


def test_lone_nested_hit_and_rule_any():
    arrays = hits([(2, 1, 350)], [], [(1, 2, 400)], [(1, 0, 300), (2, 0, 300 + 30 + 22)])
    assert chimera.flag_reads(*arrays, INFO, "junction", 100).tolist() == [False, False, False, True]
    assert chimera.flag_reads(*arrays, INFO, "any", 100).tolist() == [True, False, True, True]
    with pytest.raises(ValueError):
        chimera.flag_reads(*arrays, INFO, "some", 100)


def test_second_stored_hit_can_make_the_junction_and_unstored_hits_cannot():
    arrays = hits([(1, 0, 150), (1, 0, 500), (0, 0, 540)], [(1, 0, 150), (1, 0, 300), (1, 0, 500), (0, 0, 540)])
    # read 1 has three `-` hits: only the first H = 2 are stored, the one at 500 is not
    assert chimera.flag_reads(*arrays, INFO, "junction", 100).tolist() == [True, False]


def test_report_bytes():
    nhit, dist, end = hits([], [(1, 0, 353), (0, 1, 401)], [(2, 2, 120), (2, 0, 290), (2, 1, 400)])
    flagged = chimera.flag_reads(nhit, dist, end, INFO, "junction", 100)
    assert flagged.tolist() == [False, True, False]
    rows = chimera.report_rows(["r0", "r1", "r2"], [500, 700, 650], nhit, dist, end, INFO, flagged)
    assert chimera.REPORT_HEADER + "".join(rows) == (
        "read_id\tlength\tprimer\tstrand\tdistance\tend\tread_flagged\n"
        "r1\t700\tP1\t+\t1\t401\t1\n"
        "r1\t700\tP1\t-\t0\t353\t1\n"
        "r2\t650\tP2\t+\t2\t120\t0\n"
        "r2\t650\tP2\t+\t0\t290\t0\n")


def test_panel_patterns_of_the_golden_panel():
    ns = argparse.Namespace(primer_file=f"{GOLDEN}/primers.fasta", specimen_file=f"{GOLDEN}/specimens.txt",
                            index_edit_distance=-1, primer_edit_distance=-1, search_len=80)
    specimens, parameters = chimera.load_panel(ns)
    info = chimera.panel_patterns(specimens, parameters, 3)
    primers = list(specimens._primers.values())
    assert len(info) == 2 * len(primers) >= 6
    for i, p in enumerate(primers):
        assert info[2 * i] == PatternInfo(p.name, "+", p.primer, 3)
        assert info[2 * i + 1] == PatternInfo(p.name, "-", p.primer_rc, 3)
    assert {p.name for p in primers} >= {"ITS1F", "ITS4", "gITS7"}
    # the demux threshold caps the inner one: -E 1 means 1 here too
    ns.primer_edit_distance = 1
    specimens, parameters = chimera.load_panel(ns)
    assert {p.k for p in chimera.panel_patterns(specimens, parameters, 3)} == {1}
    assert {p.k for p in chimera.panel_patterns(specimens, parameters, 0)} == {0}


def test_option_parsing():
    a = chimera.parse_args(["p.fasta", "s.txt", "r.fastq"])
    assert (a.inner_edit_distance, a.junction_gap, a.flag_rule, a.search_len, a.max_hits) == (3, 100, "junction", 80, 4)
    assert (a.start_seq, a.num_seqs, a.primer_edit_distance, a.report, a.clean, a.flagged) == (1, -1, -1, None, None, None)
    a = chimera.parse_args(["p.fasta", "s.txt", "r.fastq.gz", "-E", "5", "-l", "60", "-n", "10", "--inner-edit-distance", "2",
                            "--junction-gap", "40", "--flag-rule", "any", "--report", "x.tsv", "--clean", "c.fq",
                            "--flagged", "f.fq"])
    assert (a.primer_edit_distance, a.search_len, a.num_seqs, a.inner_edit_distance, a.junction_gap, a.flag_rule) == \
        (5, 60, 10, 2, 40, "any")
    assert (a.report, a.clean, a.flagged) == ("x.tsv", "c.fq", "f.fq")
    assert chimera.parse_args(["p", "s", "r", "-n", "5,7"]).start_seq == 5
    for bad in (["--flag-rule", "none"], ["--inner-edit-distance", "-1"], ["--junction-gap", "-2"], ["--max-hits", "9"],
                ["-n", "x"]):
        with pytest.raises(SystemExit):
            chimera.parse_args(["p", "s", "r", *bad])


def _split(path, tmp_path, pick, batch_reads=1000):
    """The file through the native reader in batches of batch_reads; record i goes to the flagged file when pick(i)."""
    from specimux_amd.native_io import Reader
    clean, flagged = tmp_path / "clean.out", tmp_path / "flagged.out"
    for p in (clean, flagged):
        open(p, "wb").close()
    reader = Reader(str(path))
    done = 0
    while True:
        batch = reader.next_batch(batch_reads)
        if batch is None:
            break
        flags = np.array([pick(done + i) for i in range(len(batch))], dtype=np.uint8)
        batch.write_split(flags, str(clean), str(flagged))
        done += len(batch)
        batch.close()
    reader.close()
    return clean.read_bytes(), flagged.read_bytes(), done


def test_split_writes_the_input_records_byte_for_byte(tmp_path):
    src = f"{GOLDEN}/sequences.fastq"
    with open(src, "rb") as fh:
        lines = fh.read().split(b"\n")
    raw = [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]
    assert len(raw) == 40 and all(len(rec.split(b"\n")[0].split()) > 1 for rec in raw)
    pick = lambda i: i % 7 == 2
    for path, batch_reads in ((src, 1000), (src, 7)):                       # one batch, and six
        clean, flagged, n = _split(path, tmp_path, pick, batch_reads)
        assert n == 40
        assert clean == b"".join(r for i, r in enumerate(raw) if not pick(i))
        assert flagged == b"".join(r for i, r in enumerate(raw) if pick(i))
    gz = tmp_path / "sequences.fastq.gz"
    with gzip.open(gz, "wb") as fh:
        fh.write(b"".join(raw))
    clean, flagged, _ = _split(gz, tmp_path, pick)
    assert clean + flagged == b"".join([r for i, r in enumerate(raw) if not pick(i)] + [r for i, r in enumerate(raw) if pick(i)])


def test_split_irregular_fastq_fasta_and_high_bytes(tmp_path):
    from specimux_amd.native_io import Reader
    # a wrapped record sends the file to the general reader; titles keep their description and bytes above 0x7f, lose only
    # trailing white space; sequence and quality come out on one line each
    fq = tmp_path / "odd.fastq"
    fq.write_bytes(b"@r1 runid=\xe9\x80 ch=5  \r\nACGT\nAC\n+\nIIII\nII\n@r2\nTTTT\n+r2\nJJJJ\n")
    clean, flagged, n = _split(fq, tmp_path, lambda i: i == 1)
    assert n == 2 and clean == b"@r1 runid=\xe9\x80 ch=5\nACGTAC\n+\nIIIIII\n" and flagged == b"@r2\nTTTT\n+\nJJJJ\n"
    fa = tmp_path / "reads.fasta"
    fa.write_bytes(b">s1 first one\nACGT\nACGT\n>s2\nGG\n")
    clean, flagged, n = _split(fa, tmp_path, lambda i: i == 0)
    assert n == 2 and flagged == b">s1 first one\nACGTACGT\n" and clean == b">s2\nGG\n"
    reader = Reader(str(fq))
    batch = reader.next_batch(10)
    assert batch.title(0) == b"r1 runid=\xe9\x80 ch=5" and batch.title(1) == b"r2" and batch.record(0)[0] == "r1"
    batch.write_split(np.zeros(2, dtype=np.uint8), None, str(tmp_path / "none.out"))     # clean side dropped
    assert (tmp_path / "none.out").read_bytes() == b""
    batch.close()
    reader.close()
