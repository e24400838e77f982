"""CPU simulation of the error-profile kernel (specimux_amd/csrc/smx_profile.hip): its body as a host loop
(tests/cpu/profile_host.h) over the host/device core smx_profile_core.h and the plans of smx_cons_plan.h, against plain
loops over the rows.  The counters the simulation prints are bounded from below so that its coverage cannot shrink
unnoticed.  And the arguments smx_cons_profile refuses are refused by host code alone.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("profile") / "profile_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", exe, os.path.join(REPO, "tests", "cpu", "profile_sim.cpp")])
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


def test_every_row_of_short_drafts(sim):
    """16 choices per column -- match, sub, del, other x an insertion of 0, 1, 2 or 5 bases before it -- and 4 for the
    insertion behind the last base: 4 * 16^m rows per draft of m columns, over 2 + 3 + 4 + 5 drafts of 1..4 columns."""
    c = run(sim, "exhaustive")
    assert c["jobs"] == 14
    assert c["rows"] == c["members"] == 4 * (2 * 16 + 3 * 16**2 + 4 * 16**3 + 5 * 16**4)
    assert c["columns"] == 4 * (2 * 16 + 3 * 2 * 16**2 + 4 * 3 * 16**3 + 5 * 4 * 16**4)
    # a quarter of the columns each where the draft's byte is a base; an `N` column is other whatever the member has
    assert c["dels"] * 4 == c["columns"] and c["subs"] < c["dels"] < c["others"]
    assert c["ins_events"] * 4 > c["columns"] * 3              # three of four words carry an insertion, word m included
    assert c["ins_beyond_kept"] * 3 == c["ins_events"]         # one insertion in three has five bases: one beyond the kept
    assert c["runs_at_clamp"] > 10000 and c["members_empty"] > 1000 and c["q_bin_0"] > 10**6 and c["q_bin_63"] > 10**6


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_profile_jobs_against_plain_loops(sim, seed):
    c = run(sim, "random", str(seed))
    assert c["calls"] == 12 and c["jobs"] >= 45 and c["jobs_without_members"] >= 5
    assert c["members"] >= 1000 and c["members_above_limit"] >= 100 and c["members_clipped"] >= 100
    assert c["columns"] >= 100000 and c["subs"] >= 4000 and c["dels"] >= 4000 and c["others"] >= 500 and c["ins_events"] >= 2500
    assert c["ins_beyond_kept"] >= 30000 and c["q_bases"] >= 90000 and c["q_bin_0"] >= 10000 and c["q_bin_63"] >= 30000
    assert c["runs_seen"] >= 25000 and c["runs_class_8"] >= 3000 and c["runs_at_clamp"] >= 1500 and c["runs_across_batches"] >= 800


# ------------------------------------------------------------------------------------------------ the refusals
def test_null_profile_arguments_are_refused_before_the_device_is_asked():
    """A null quals, per_member or tables beside members is SMX_ERR_ARG from host code alone: on a machine without a GPU
    the same call with good arguments is the one that fails, with SMX_ERR_DEVICE.  No output is touched.  The checks of
    the jobs come with the plan, as for smx_cons_votes."""
    import torch
    from specimux_amd import _lib, calls
    lib = _lib.load()
    reads = [b"ACGTACGT", b"ACGAACGT", b"", b"ACGT", b"ACGTT"]
    quals = b"".join(b"I" * len(r) for r in reads)
    roff = calls.offsets(reads)
    ks = np.array([2] * len(reads), dtype=np.int32)
    mark = 0x5A5A5A5A

    def call(jobs, null=()):
        jarr = calls.job_array(jobs, _lib.CONS_JOB_DTYPE)
        outs = [np.full(n, mark, dtype=np.uint32) for n in (4096, 8, 64, 3 * 274)]
        rc = lib.smx_cons_profile(b"".join(reads), _lib.ptr(roff), len(reads), _lib.ptr(ks), _lib.ptr(jarr), len(jobs),
                                  None if "quals" in null else quals, _lib.ptr(outs[0]), _lib.ptr(outs[1]),
                                  None if "per_member" in null else _lib.ptr(outs[2]), None if "tables" in null else _lib.ptr(outs[3]),
                                  None)
        return rc, lib.smx_last_error().decode(), all((o == mark).all() for o in outs)
    good = [(0, 0, 2), (3, 2, 0), (0, 2, 3)]
    for name in ("quals", "per_member", "tables"):
        rc, msg, untouched = call(good, null=(name,))
        assert rc == _lib.ERR_ARG and name in msg and "5 members" in msg and untouched, (name, msg)
    rc, msg, untouched = call([(2, 0, 2)])
    assert rc == _lib.ERR_ARG and "empty draft" in msg and untouched
    rc, msg, untouched = call([(0, 0, 3), (3, 2, 2)])
    assert rc == _lib.ERR_ARG and "overlap" in msg and untouched
    rc, msg, _ = call(good)
    assert rc == (_lib.OK if torch.cuda.is_available() else _lib.ERR_DEVICE), msg
    assert call([])[0] == _lib.OK and call([], null=("quals", "per_member", "tables"))[0] == _lib.OK
    # the three may be null where no job has members: the device is asked, and nothing is read
    rc, msg, _ = call([(3, 2, 0)], null=("quals", "per_member"))
    assert rc == (_lib.OK if torch.cuda.is_available() else _lib.ERR_DEVICE), msg
