"""specimux-identify on the GPU: the tool run over the synthetic database of tests/identify_utils.py on the device and
with the oracle in place of the device call writes the same --report and --json files byte for byte, with the database
in one piece and in three."""
import json
import os

import pytest

from specimux_amd import identify

import identify_utils as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = os.fspath(tmp_path_factory.mktemp("identify"))
    queries, refs = U.build_files(root)
    return root, queries, refs


@pytest.mark.parametrize("pieces", [1, 3])
def test_device_and_oracle_write_the_same_files(tree, tmp_path, monkeypatch, pieces):
    root, queries, refs = tree
    if pieces == 3:
        monkeypatch.setenv("SMX_IDENTIFY_BUDGET_BYTES", str(U.three_piece_budget(queries, refs)))
    else:
        monkeypatch.delenv("SMX_IDENTIFY_BUDGET_BYTES", raising=False)
    dev, ora = os.fspath(tmp_path / "dev"), os.fspath(tmp_path / "ora")
    ms = []
    assert identify.run(U.args_for(root, dev), kernel_ms=ms) == 0
    assert identify.run(U.args_for(root, ora), hits_fn=identify.best_hits_oracle) == 0
    assert len(ms) == pieces and min(ms) > 0
    got, want = U.outputs(dev), U.outputs(ora)
    assert got["report.tsv"] == want["report.tsv"] and got["report.json"] == want["report.json"]
    doc = json.loads(got["report.json"])
    assert doc["summary"] == {"queries": 8, "refs": len(refs), "unique": 5, "tied": 1, "none": 2, "device_calls": pieces}
    rows = U.rows_of(got["report.tsv"])
    assert rows["Q_RC"][0]["strand"] == "-" and rows["Q_TRIM"][0]["pattern"] == "ref" and rows["Q_FLANK"][0]["pattern"] == "query"
