"""specimux-bimera on the GPU: the tool run over the synthetic plate of tests/bimera_utils.py on the device and with the
plain-Python twin in place of the device call; TSV, JSON and the cleaned FASTA must be byte-identical, in both scopes, with
and without --parents, under a budget that cuts the pool into three pieces."""
import argparse

import pytest

import bimera_utils as U
from specimux_amd import bimera

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plate():
    return U.Plate()


def outputs(tmp_path, tag, reach_fn, kernel_ms=None, **kw):
    base = dict(consensus=None, fasta=None, parents=None, scope="specimen", max_edits=U.MAX_EDITS, min_gain=U.MIN_GAIN,
                min_parent_ratio=2.0, report=str(tmp_path / f"{tag}.tsv"), json=str(tmp_path / f"{tag}.json"),
                clean=str(tmp_path / f"{tag}.fasta"), debug=False)
    base.update(kw)
    args = argparse.Namespace(**base)
    assert (bimera.run(args, kernel_ms=kernel_ms) if reach_fn is None else bimera.run(args, reach_fn=reach_fn)) == 0
    return tuple(open(p, "rb").read() for p in (args.report, args.json, args.clean))


@pytest.mark.parametrize("scope", ["specimen", "plate"])
def test_the_device_gives_the_twins_files(tmp_path, plate, scope):
    src = tmp_path / "consensus.json"
    src.write_text(plate.consensus_json())
    ms = []
    got = outputs(tmp_path, "gpu", None, kernel_ms=ms, consensus=str(src), scope=scope)
    want = outputs(tmp_path, "twin", U.keys_reference, consensus=str(src), scope=scope)
    assert got == want
    assert got[0].count(b"\tchimera\t") == (6 if scope == "specimen" else 8)
    assert len(ms) == 1 and ms[0] > 0.0


def test_the_device_gives_the_twins_files_with_a_pool(tmp_path, plate, monkeypatch):
    keep = [c for c in plate.called if plate.truth[c.name][0] != "species"]
    src = tmp_path / "called.fasta"
    src.write_text("".join(f">{c.title}\n{c.seq}\n" for c in keep))
    pool = tmp_path / "parents.fasta"
    pool.write_text("".join(f">{c.name} voucher\n{c.seq}\n" for c in plate.called if plate.truth[c.name][0] == "species"))
    want = outputs(tmp_path, "twin", U.keys_reference, fasta=str(src), parents=str(pool), scope="plate")
    ms = []
    assert outputs(tmp_path, "gpu", None, kernel_ms=ms, fasta=str(src), parents=str(pool), scope="plate") == want
    assert len(ms) == 2
    monkeypatch.setenv("SMX_BIMERA_BUDGET_BYTES", str(sum(len(c.seq) for c in keep) + 4 * 160 + 10))
    ms = []
    pieces = outputs(tmp_path, "pieces", None, kernel_ms=ms, fasta=str(src), parents=str(pool), scope="plate")
    assert len(ms) == 4                            # the run's own call, then three pieces of the pool
    assert pieces[0] == want[0] and pieces[2] == want[2]
    assert pieces[1].replace(b'"device_calls": 4', b'"device_calls": 2') == want[1]
    assert want[0].count(b"\tchimera\t") == 8
