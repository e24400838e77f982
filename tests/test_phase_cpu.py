"""CPU simulation of the variant kernels' shared code (specimux_amd/csrc/smx_phase_core.h: the host/device functions the
gfx950 kernels of smx_phase.hip run): the site rule, the classification of a row word, the plane words and the link counts
against plain loops over pileup rows from the full-matrix reference walk.  The counters the simulation prints are bounded
from below so that its coverage cannot shrink unnoticed.  And the arguments smx_cons_phase refuses are refused by host
code alone.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("phase") / "phase_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", exe, os.path.join(REPO, "tests", "cpu", "phase_sim.cpp")])
    return exe


def run(sim, *args):
    out = subprocess.run([sim, *args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.rstrip().endswith("\n0 mismatches"), out.stdout[-4000:]
    counts = {}
    for line in out.stdout.splitlines():
        key, _, val = line.partition(" ")
        if val.lstrip("-").isdigit() and key.isidentifier():
            counts[key] = int(val)
    return counts


def test_phase_rules_exhaustive(sim):
    c = run(sim, "exhaustive")
    assert c["base_vectors"] == 4096 and c["base_tie_major"] > 1000 and c["base_tie_minor"] > 1000
    assert c["base_other_largest"] > 250                       # "other" has the most votes and is still ignored
    assert c["ins_vectors"] == 5 * sum((p + 1) for a in range(13) for p in range(a + 1)) and c["ins_tie"] > 100
    assert c["threshold_cases"] == 4 * 12 * sum(a + 1 for a in range(41))
    assert c["on_share_threshold"] > 300 and c["on_count_threshold"] > 1500
    assert c["classified"] == 8 * 4 * 2 * (20 + 2)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_phase_jobs_against_plain_loops(sim, seed):
    c = run(sim, "random", str(seed))
    assert c["jobs"] == 61 and c["sites_kept"] >= 250 and c["jobs_clipped"] >= 10
    assert c["sites_base"] >= 150 and c["sites_ins"] >= 40 and c["sites_deletion"] >= 15
    assert c["sites_at_0"] >= 15 and c["sites_at_m"] >= 5 and c["sites_at_m_minus_1"] >= 10
    assert c["members_above_limit"] >= 300 and c["positions_with_other"] >= 500
    assert c["plane_bits"] >= 20000 and c["plane_neither"] >= 300
    assert c["link_pairs"] >= 1000 and c["link_pairs_with_gaps"] >= 500


def test_bad_phase_arguments_are_refused_before_the_device_is_asked():
    """max_sites of 0 or above 64 and min_permille above 1000 are SMX_ERR_ARG from host code alone: on a machine without
    a GPU the same call with good arguments is the one that fails, with SMX_ERR_DEVICE.  The checks of the jobs come
    with the plan, as for smx_cons_votes."""
    import torch
    from specimux_amd import _lib, calls
    lib = _lib.load()
    reads = [b"ACGTACGT", b"ACGAACGT", b"", b"ACGT", b"ACGTT"]
    roff = calls.offsets(reads)
    ks = np.array([2] * len(reads), dtype=np.int32)

    def call(jobs, min_permille, min_reads, max_sites):
        jarr = np.array(jobs, dtype=_lib.CONS_JOB_DTYPE)
        votes, aligned = np.zeros(4096, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
        sites = np.zeros(8 * 64, dtype=_lib.CONS_SITE_DTYPE)
        n_sites, n_qualified = np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
        planes, link = np.zeros(8 * 128, dtype=np.uint64), np.zeros(8 * 64 * 64 * 4, dtype=np.uint32)
        rc = lib.smx_cons_phase(b"".join(reads), _lib.ptr(roff), len(reads), _lib.ptr(ks), _lib.ptr(jarr), len(jobs),
                                min_permille, min_reads, max_sites, _lib.ptr(votes), _lib.ptr(aligned), _lib.ptr(sites),
                                _lib.ptr(n_sites), _lib.ptr(n_qualified), _lib.ptr(planes), _lib.ptr(link), None)
        return rc, lib.smx_last_error().decode()
    good = [(0, 0, 2), (3, 2, 0), (0, 2, 3)]
    for max_sites in (0, 65, 2**32 - 1):
        rc, msg = call(good, 150, 2, max_sites)
        assert rc == _lib.ERR_ARG and "max_sites" in msg, (max_sites, msg)
    rc, msg = call(good, 1001, 2, 8)
    assert rc == _lib.ERR_ARG and "min_permille" in msg
    rc, msg = call([], 1001, 2, 8)                             # refused even where there is nothing to do
    assert rc == _lib.ERR_ARG and "min_permille" in msg
    rc, msg = call([(2, 0, 2)], 150, 2, 8)
    assert rc == _lib.ERR_ARG and "empty draft" in msg
    rc, msg = call([(0, 0, 3), (3, 2, 2)], 150, 2, 8)
    assert rc == _lib.ERR_ARG and "overlap" in msg
    for max_sites, min_permille in ((1, 0), (64, 1000)):
        rc, msg = call(good, min_permille, 2, max_sites)
        assert rc == (_lib.OK if torch.cuda.is_available() else _lib.ERR_DEVICE), msg
    assert call([], 150, 2, 8)[0] == _lib.OK
