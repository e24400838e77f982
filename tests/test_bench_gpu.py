"""bench.py at a small size: a plain run prints the headline line and does none of the wider measurements; --full adds
them.  The JSON line's own numbers must agree with each other and with the dumped counts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

READS, STEPS = 20_000, 2
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
WIDE = ("step_kernels", "one_stream", "single_buffer", "cpu_baseline", "other_configs", "pcie_inclusive", "end_to_end")


def run_bench(*args):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
                        "--reads", str(READS), *args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_headline_only(tmp_path):
    from specimux_amd import _lib
    out = run_bench("--dump-outputs", str(tmp_path))
    assert all(k in out for k in HEADLINE)
    assert out["unit"] == "reads/s" and out["higher_is_better"] is True and out["dtype"] == "u32"
    assert out["value"] * out["ms_per_step"] * 1e-3 == pytest.approx(READS, rel=1e-9)
    assert not [k for k in WIDE if k in out]
    assert "dominant_kernel" not in out["roofline"]
    counts = np.load(tmp_path / "counts.npy")
    assert counts[_lib.CNT_TOTAL] == READS * STEPS and counts[_lib.CNT_OVERFLOW] == 0


def test_full_run_adds_the_wider_scopes():
    out = run_bench("--full", "--no-extras")
    assert all(k in out for k in HEADLINE)
    assert [k["kernel"] for k in out["step_kernels"]][:2] == ["smx::prescan_transpose_kernel", "smx::prescan_dp_kernel"]
    assert all(k["ms"] > 0 for k in out["step_kernels"])
    assert out["one_stream"]["ms_per_step"] > 0 and out["single_buffer"]["ms_per_step"] > 0
    assert out["roofline"]["dominant_kernel"]["kernel_ms_avg"] == out["step_kernels"][2]["ms"]
    assert out["cpu_baseline"]["value"] > 0 and out["gpu_over_cpu"] > 0
    assert not [k for k in ("other_configs", "pcie_inclusive", "end_to_end") if k in out]
