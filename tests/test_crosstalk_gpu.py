"""specimux-crosstalk on the GPU: the tool run over the synthetic run of tests/crosstalk_utils.py on the device and with
the oracle in place of the device call writes the same --report, --json and --reads files byte for byte, with all reads
and with --max-reads 20; two device calls under a small budget change nothing but the call count."""
import json
import os

import pytest

from specimux_amd import crosstalk

import crosstalk_utils as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("crosstalk_run")
    U.build_run(os.fspath(root))
    return root


@pytest.mark.parametrize("max_reads", [0, 20])
def test_device_and_oracle_write_the_same_files(run_tree, tmp_path, max_reads):
    dev, ora = os.fspath(tmp_path / "dev"), os.fspath(tmp_path / "ora")
    ms = []
    assert crosstalk.run(U.args_for(run_tree, dev, max_reads=max_reads), kernel_ms=ms) == 0
    assert crosstalk.run(U.args_for(run_tree, ora, max_reads=max_reads), nearest_fn=crosstalk.nearest_oracle) == 0
    assert len(ms) == 1 and ms[0] > 0
    got, want = U.outputs(dev), U.outputs(ora)
    for name in want:
        assert got[name] == want[name], name
    doc = json.loads(want["report.json"])
    assert doc["summary"]["reads"] == (118 if max_reads == 0 else 20 * 5 + 5)
    if max_reads == 0:
        assert doc["summary"]["flagged_sources"] == 2 and doc["summary"]["foreign"] == 11


def test_two_device_calls_change_nothing(run_tree, tmp_path, monkeypatch):
    one, two = os.fspath(tmp_path / "one"), os.fspath(tmp_path / "two")
    assert crosstalk.run(U.args_for(run_tree, one)) == 0
    # the refs and half of the files: two calls
    sizes = sum(os.path.getsize(p) for p in crosstalk.specimine.discover_specimens(os.fspath(run_tree)))
    monkeypatch.setenv("SMX_CLUSTERS_BUDGET_BYTES", str(6 * 300 + sizes * 2 // 3))
    ms = []
    assert crosstalk.run(U.args_for(run_tree, two), kernel_ms=ms) == 0
    assert len(ms) == 2
    a, b = U.outputs(one), U.outputs(two)
    assert a["report.tsv"] == b["report.tsv"] and a["reads.tsv"] == b["reads.tsv"]
    da, db = json.loads(a["report.json"]), json.loads(b["report.json"])
    assert (da["summary"]["device_calls"], db["summary"]["device_calls"]) == (1, 2)
    db["summary"]["device_calls"] = 1
    assert da == db
