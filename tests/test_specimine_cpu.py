"""specimine host logic without a GPU: arguments, specimen ids, index lookup, input level, partial-file discovery,
the record title and the k formula (reference src/specimux/specimine.py)."""
import glob
import logging
import os

import pytest

from specimux_amd import cli, specimine
from specimux_amd.io_utils import SeqRecord


def touch(path, text=""):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text)


def test_argument_defaults_and_flags():
    a = specimine.parse_arguments(["--index", "i.txt", "--fastq", "f.fastq"])
    assert (a.index, a.fastq, a.partial_forward, a.no_partial_reverse, a.min_identity, a.debug) == \
        ("i.txt", "f.fastq", False, False, 0.85, False)
    a = specimine.parse_arguments(["--index", "i", "--fastq", "f", "--partial-forward", "--no-partial-reverse",
                                   "--min-identity", "0.5", "--debug"])
    assert (a.partial_forward, a.no_partial_reverse, a.min_identity, a.debug) == (True, True, 0.5, True)
    with pytest.raises(SystemExit):
        specimine.parse_arguments(["--fastq", "f"])
    with pytest.raises(SystemExit):
        specimine.parse_arguments(["--index", "i"])
    assert callable(cli.specimine_main)


def test_extract_specimen_id():
    assert specimine.extract_specimen_id("/x/full/P/ABC_1.fastq") == "ABC_1"
    assert specimine.extract_specimen_id("sample_ABC.fastq") == "ABC"
    assert specimine.extract_specimen_id("ABC.fastq.gz") == "ABC"     # re.match: a prefix match is enough
    with pytest.raises(ValueError):
        specimine.extract_specimen_id("/x/full/P/ABC.fasta")


def test_find_barcodes(tmp_path, caplog):
    named = tmp_path / "named.txt"
    named.write_text("RvIndex\tSampleID\tFwIndex\nttgg\tS1\tacgt\nGGGG\tS2\tCCCC\nAAAA\tS1\tTTTT\n")
    assert specimine.find_barcodes("S1", str(named)) == ("ACGT", "TTGG")      # first row, upper case
    assert specimine.find_barcodes("S2", str(named)) == ("CCCC", "GGGG")
    default = tmp_path / "default.txt"
    default.write_text("a\tb\tc\td\te\nS9\tpool\taaaa\tp1\tcccc\nshort\trow\n")
    assert specimine.find_barcodes("S9", str(default)) == ("AAAA", "CCCC")
    with caplog.at_level(logging.ERROR):
        assert specimine.find_barcodes("S3", str(default)) == (None, None)
        assert specimine.find_barcodes("short", str(default)) == (None, None)
    assert "Could not find specimen S3" in caplog.text


def test_detect_input_level(tmp_path):
    root = str(tmp_path)
    assert specimine.detect_input_level(f"{root}/full/POOL/S.fastq") == (root, "POOL", None)
    assert specimine.detect_input_level(f"{root}/full/POOL/A-B/S.fastq") == (root, "POOL", "A-B")
    with pytest.raises(ValueError):
        specimine.detect_input_level(f"{root}/full/S.fastq")
    with pytest.raises(ValueError):
        specimine.detect_input_level(f"{root}/full/a/b/c/S.fastq")
    with pytest.raises(ValueError):
        specimine.detect_input_level(f"{root}/nofull/S.fastq")
    # the FIRST `full` component counts: here .../full/run/full/POOL/S.fastq is four levels below it
    with pytest.raises(ValueError):
        specimine.detect_input_level(f"{root}/full/run/full/POOL/S.fastq")
    assert specimine.detect_input_level(f"{root}/full/run/full/S.fastq") == (root, "run", "full")


def test_partial_files_pair_level_and_legacy_names(tmp_path):
    root = str(tmp_path)
    touch(f"{root}/partial/P/A-B/sample_barcode_fwd_F1.fastq")
    touch(f"{root}/partial/P/A-B/barcode_rev_R1.fastq")
    touch(f"{root}/partial/P/A-B/sample_barcode_rev_R1.fastq")     # the current name wins
    touch(f"{root}/partial/P/C-D/barcode_fwd_F1.fastq")            # another pair: not searched at pair level
    got = specimine.derive_partial_match_filenames(f"{root}/full/P/A-B/S.fastq", "F1", "R1")
    assert got == {"forward": [f"{root}/partial/P/A-B/sample_barcode_fwd_F1.fastq"],
                   "reverse": [f"{root}/partial/P/A-B/barcode_rev_R1.fastq"]}
    assert list(got) == ["forward", "reverse"]


def test_partial_files_pool_level_in_glob_order(tmp_path, caplog):
    root = str(tmp_path)
    for pair in ("Z-Y", "A-B", "M-N"):
        touch(f"{root}/partial/P/{pair}/barcode_fwd_F1.fastq")
    touch(f"{root}/partial/P/M-N/sample_barcode_rev_R1.fastq")
    touch(f"{root}/partial/P/not_a_dir.fastq")
    got = specimine.derive_partial_match_filenames(f"{root}/full/P/S.fastq", "F1", "R1")
    order = [d for d in glob.glob(os.path.join(root, "partial", "P", "*")) if os.path.isdir(d)]
    assert got["forward"] == [os.path.join(d, "barcode_fwd_F1.fastq") for d in order]
    assert got["reverse"] == [f"{root}/partial/P/M-N/sample_barcode_rev_R1.fastq"]
    with caplog.at_level(logging.WARNING):
        got = specimine.derive_partial_match_filenames(f"{root}/full/P/S.fastq", "F1", "R9")
    assert list(got) == ["forward"]
    assert "No reverse partial match files found for barcode: R9" in caplog.text
    assert specimine.derive_partial_match_filenames(f"{root}/full/Q/S.fastq", "F1", "R1") == {}


def _tree(root, with_fwd=True, with_rev=True):
    touch(f"{root}/index.txt", "SampleID\tPrimerPool\tFwIndex\tFwPrimer\tRvIndex\tRvPrimer\nS1\tP\tff\ta\trr\tb\n")
    touch(f"{root}/full/P/S1.fastq", "@r1\nACGT\n+\nIIII\n")
    if with_fwd:
        touch(f"{root}/partial/P/A-B/barcode_fwd_FF.fastq", "@p1\nACGT\n+\nIIII\n")
    if with_rev:
        touch(f"{root}/partial/P/A-B/barcode_rev_RR.fastq", "@p2\nACGT\n+\nIIII\n")


def test_plan_job_flag_filtering(tmp_path):
    root = str(tmp_path)
    _tree(root)
    fq = f"{root}/full/P/S1.fastq"
    assert list(specimine.plan_job(f"{root}/index.txt", fq).partial_files) == ["reverse"]
    assert list(specimine.plan_job(f"{root}/index.txt", fq, partial_forward=True).partial_files) == ["forward", "reverse"]
    job = specimine.plan_job(f"{root}/index.txt", fq, partial_forward=True, no_partial_reverse=True, min_identity=0.7)
    assert list(job.partial_files) == ["forward"] and job.min_identity == 0.7 and job.output == fq + ".mined"
    with pytest.raises(SystemExit) as e:
        specimine.plan_job(f"{root}/index.txt", fq, no_partial_reverse=True)
    assert e.value.code == 1


def test_exit_1_without_partials_or_barcodes(tmp_path):
    root = str(tmp_path)
    _tree(root, with_fwd=True, with_rev=False)
    with pytest.raises(SystemExit) as e:   # forward exists but is not selected, reverse does not exist
        specimine.main(["--index", f"{root}/index.txt", "--fastq", f"{root}/full/P/S1.fastq"])
    assert e.value.code == 1
    touch(f"{root}/full/P/S2.fastq", "@r1\nACGT\n+\nIIII\n")
    with pytest.raises(SystemExit) as e:   # specimen not in the index
        specimine.main(["--index", f"{root}/index.txt", "--fastq", f"{root}/full/P/S2.fastq", "--partial-forward"])
    assert e.value.code == 1
    assert not os.path.exists(f"{root}/full/P/S1.fastq.mined")


def test_record_title_with_and_without_description():
    rec = SeqRecord("ACGT", "read1", "read1 rc=1 pool=P", "IIII")
    title = specimine.mined_title(rec, "forward", 0.8765)
    assert title == "read1_mined_forward_0.88 read1 rc=1 pool=P mined_forward identity=0.88"
    assert specimine.format_record(title, rec) == f"@{title}\nACGT\n+\nIIII\n"
    bare = SeqRecord("AC", "r2", "r2", "!#")
    assert specimine.mined_title(bare, "reverse", 1.0) == "r2_mined_reverse_1.00 r2 mined_reverse identity=1.00"
    assert specimine.mined_title(bare, "reverse", 0.845) == "r2_mined_reverse_0.84 r2 mined_reverse identity=0.84"


def test_k_formula_and_identity():
    assert specimine.max_distance(650, 0.85) == int(650 * (1 - 0.85)) == 97
    assert specimine.max_distance(100, 1.0) == 0
    assert specimine.max_distance(100, 0.0) == 100
    assert specimine.max_distance(100, 1.5) == -50          # negative: edlib runs without a limit
    assert specimine.max_distance(100, 1.001) == 0          # int() truncates towards zero
    assert specimine.calculate_identity({"editDistance": -1}, 100) == 0
    assert specimine.calculate_identity({"editDistance": 15}, 100) == 1 - 15 / 100


def _rounding_case():
    """The first (len, min_identity) on a grid where d == k passes the k limit but 1 - d/len < min_identity."""
    for m in range(1, 400):
        for step in range(1, 100):
            mi = step / 100
            k = int(m * (1 - mi))
            if k >= 0 and 1 - k / m < mi:
                return m, mi, k
    return None


def test_k_float_rounding_case_pinned():
    case = _rounding_case()
    assert case == (5, 0.2, 4)
    m, mi, k = case
    assert specimine.max_distance(m, mi) == k == 4       # 5 * 0.8 = 4.0: a distance of 4 passes the limit
    assert 1 - (k / m) == 0.19999999999999996 < mi       # ... yet its identity is below 0.2: never mined
