"""CPU twin of the alignment kernels behind smx_align and smx_align_batch (specimux_amd/csrc/smx_align.hip): their lane
bodies (smx_align_lane.h, the same source lines) compiled for the host and held against a plain full-matrix DP by
tests/cpu/align_sim.cpp, over buffers of exactly the sizes the calls allocate.  The counters the simulation prints are
bounded from below so that its coverage cannot shrink unnoticed; every bound follows from how the cases are built (or, where
it says so, from the reference DP), none from what the lane bodies return.  The simulation's reference is itself pinned to
oracle.edlib_semantics.  And the arguments the two calls refuse are refused by host code alone.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("align") / "align_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(REPO, "specimux_amd", "csrc"),
                           "-I", os.path.join(REPO, "include"), "-o", exe, os.path.join(REPO, "tests", "cpu", "align_sim.cpp")])
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
    assert counts["iupac_pairs"] == 28          # the Peq tables' alphabet against the list of pairs, before anything runs
    return counts, out.stdout


def test_exhaustive_small_alignments(sim):
    c, _ = run(sim, "exhaustive")
    n_targets = sum(4 ** n for n in range(1, 8))
    # queries over {A, C, N, x}: those with an `x` are refused by build_peq, the others run
    assert c["queries"] == sum(3 ** m for m in range(1, 5)) == 120 and c["queries_refused"] == sum(4 ** m - 3 ** m for m in range(1, 5))
    assert c["cases"] == 120 * n_targets * 2 * 6
    # k = 0..5 against m = 1..4: 3^m queries have 6 - m values of k >= m, in each mode
    k_ge_m = sum(3 ** m * (6 - m) for m in range(1, 5)) * n_targets
    assert c["k_ge_m_hw"] == c["k_ge_m_shw"] == k_ge_m
    # a target of n >= 2 letters `x` matches nothing: in HW mode with k >= m every one of its n columns is optimal, so the
    # launches with cap 0 and cap 1 hold it with cap < nloc; with k = 0 a target of `x` alone is above k in both modes
    barren = sum(3 ** m * (6 - m) for m in range(1, 5)) * 6
    assert c["several_locations"] >= barren and c["cap_below_nloc"] >= 2 * barren
    assert c["above_k"] >= 120 * 2 * 7
    # per (query, mode, k): one launch with cap 0, one with cap 1 over a workspace of 0xFF
    assert c["cap_zero_launches"] == 120 * 2 * 6 and c["dirty_workspace_launches"] >= 120 * 2 * 6


def test_byte_wide_score_column_cannot_wrap(sim):
    """A target that is the query followed by at least 256 letters of filler costs 0 at column m and 256 at column
    m + 256: a witness by construction.  Per query length: three such target lengths (m + 256, 600, 1000) for each of seven
    k, three more (m + 999 .. m + 1001) at k = 1000, and for m = 1 the length 257 once more per k: 8 * 24 + 7 = 199.  The
    simulation holds every one of them against the reference DP (`a full prefix is no witness` is a mismatch)."""
    c, _ = run(sim, "wrap")
    assert c["full_prefix_cases"] == 8 * (7 * 3 + 3) + 7 == 199
    assert c["wrap_witnesses"] >= 199
    # 8 lengths x 7 k x 10 target lengths (m + k - 1 = 0 dropped for m = 1, k = 0) x 4 targets x 2 modes; k <= 250 also in launches
    assert c["single_cases"] == (8 * 7 * 10 - 2) * 4 * 2 and c["batch_cases"] == (8 * 6 * 10 - 2) * 4 * 2
    # k in {m, 200, 249, 250, 1000} is >= m for every m <= 64
    assert c["k_ge_m_hw"] == c["k_ge_m_shw"] == 8 * 5 * 10 * 4
    # the target without a matching letter, HW, k in {m, 200, 249, 250}: every column is optimal, and cap 0 is below that
    assert c["cap_below_nloc"] >= 8 * 4 * 10 and c["cap_zero_launches"] >= 60 and c["dirty_workspace_launches"] >= 100


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_launches_against_full_matrix(sim, seed):
    """Launch sizes 1, 64, 65, 129, 400, 2, 63, 200, 400, 300, 17, 128; alignment `it` of a launch gets its plant from
    it % 4, its k from it % 8, its mode from (it / 8) % 2 and a target without a matching letter where it % 32 is 7 or 16
    (tests/cpu/align_sim.cpp: random_launch).  The bounds are counts of such `it` below the launch sizes."""
    c, _ = run(sim, "random", str(seed))
    sizes = [1, 64, 65, 129, 400, 2, 63, 200, 400, 300, 17, 128]

    def its(mod, *residues):
        return sum(1 for n in sizes for it in range(n) if it % mod in residues)
    assert c["alignments"] == sum(sizes) and c["launches"] == c["launches_repeated"] == 12
    assert c["launches_full_last_wave"] == 2 and c["launches_one_lane_in_last_wave"] == 3
    assert c["planted_at_0"] == its(4, 1) and c["planted_at_end"] == its(4, 2)
    assert c["k_ge_m_hw"] >= its(16, 5, 6, 7) > 300 and c["k_ge_m_shw"] >= its(16, 13, 14, 15) > 300 and c["k_250"] >= its(8, 7)
    assert c["no_matching_letter"] == its(32, 7, 16) == 112
    # it % 32 == 7: HW, k = 250, no matching letter, at least 17 columns -- all optimal: below cap 0, 1 and 16
    assert c["more_than_16_locations"] >= its(32, 7) and c["cap_below_nloc"] >= 3 * its(32, 7)
    assert c["above_k"] >= its(32, 16)                       # HW, k = 0, no matching letter
    assert c["shw_trimmed"] >= its(16, 8) > 100              # SHW, k = 0, target longer than the query
    assert c["targets_with_other_bytes"] >= its(32, 7, 16)
    assert c["cap_zero_launches"] >= 12 and c["dirty_workspace_launches"] >= 12 * 5


def test_the_simulations_reference_is_the_oracles(sim):
    """Some hundred cases of the three sets, with what the simulation's full-matrix DP says, against
    oracle.edlib_semantics.align."""
    from oracle import edlib_semantics as E
    c, out = run(sim, "cases")
    n = {0: 0, 1: 0}
    for line in out.splitlines():
        if not line.startswith("CASE "):
            continue
        _, q, thex, mode, k, dist, locs = line.split(" ")
        t = bytes.fromhex(thex).decode("latin-1")
        exp = E.align(q, t, E.SHW if mode == "1" else E.HW, int(k))
        got = [] if locs == "-" else [tuple(int(v) for v in p.split(":")) for p in locs.split(",")]
        assert (int(dist), got) == (exp["editDistance"], [tuple(x) for x in exp["locations"]]), line[:200]
        n[int(mode)] += 1
    assert n[0] + n[1] == c["cases_printed"] and n[0] > 200 and n[1] > 200


# ------------------------------------------------------------------------------------------------ the refusals
def test_bad_alignment_arguments_are_refused_before_the_device_is_asked():
    """Each refusal of smx_align and smx_align_batch comes from host code with its documented status (include/smx.h); on a
    machine without a GPU the same calls with good arguments are the ones that fail, with SMX_ERR_DEVICE."""
    import torch
    from specimux_amd import _lib, calls
    lib = _lib.load()
    valid = _lib.OK if torch.cuda.is_available() else _lib.ERR_DEVICE

    def single(q, t, k=1, mode=0, qlen=None, tlen=None):
        d, n = C.c_int(), C.c_int()
        rc = lib.smx_align(q, len(q) if qlen is None else qlen, t, len(t) if tlen is None else tlen, k, mode, C.byref(d), None,
                           None, 0, C.byref(n))
        return rc, lib.smx_last_error().decode()
    rc, msg = single(b"A", b"ACGT", qlen=0)
    assert rc == _lib.ERR_UNSUPPORTED and "outside 1..64" in msg
    rc, msg = single(b"A" * 65, b"ACGT")
    assert rc == _lib.ERR_UNSUPPORTED and "outside 1..64" in msg
    rc, msg = single(b"ACxT", b"ACGT")
    assert rc == _lib.ERR_UNSUPPORTED and "outside the IUPAC DNA alphabet" in msg
    rc, msg = single(b"ACGT", b"ACGT", mode=2)
    assert rc == _lib.ERR_UNSUPPORTED and "mode 2" in msg
    rc, msg = single(b"ACGT", b"ACGT", tlen=0)
    assert rc == _lib.ERR_UNSUPPORTED and "empty target" in msg
    for k in (0, 1, 64, 1000):
        assert single(b"ACGT", b"ACGTACGT", k=k)[0] == valid
    assert single(b"A" * 64, b"C")[0] == valid

    def batch(queries, targets, qidx, ks, modes, n=None):
        qoff, toff = calls.offsets(queries, np.uint32), calls.offsets(targets)
        qidx, ks, modes = np.array(qidx, dtype=np.uint32), np.array(ks, dtype=np.int32), np.array(modes, dtype=np.uint8)
        n = len(targets) if n is None else n
        dist, nloc = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        rc = lib.smx_align_batch(b"".join(queries), _lib.ptr(qoff), len(queries), b"".join(targets), _lib.ptr(toff), _lib.ptr(qidx),
                                 _lib.ptr(ks), _lib.ptr(modes), n, _lib.ptr(dist), _lib.ptr(nloc), None, None, 0)
        return rc, lib.smx_last_error().decode()
    good = ([b"ACGT", b"N"], [b"ACGTT", b"A", b"CCC"], [0, 1, 1], [1, 0, 250], [0, 1, 0])
    rc, msg = batch([b"ACGT", b""], *good[1:])
    assert rc == _lib.ERR_UNSUPPORTED and "query 1: length 0" in msg
    rc, msg = batch([b"A" * 65, b"N"], *good[1:])
    assert rc == _lib.ERR_UNSUPPORTED and "query 0: length 65" in msg
    rc, msg = batch([b"ACGT", b"x"], *good[1:])
    assert rc == _lib.ERR_UNSUPPORTED and "query 1" in msg and "outside the IUPAC DNA alphabet" in msg
    rc, msg = batch(good[0], [b"ACGTT", b"", b"CCC"], *good[2:])
    assert rc == _lib.ERR_UNSUPPORTED and "alignment 1: empty target" in msg
    rc, msg = batch(good[0], good[1], [0, 1, 2], *good[3:])
    assert rc == _lib.ERR_ARG and "alignment 2: bad query index or mode" in msg
    rc, msg = batch(*good[:4], [0, 2, 0])
    assert rc == _lib.ERR_ARG and "alignment 1: bad query index or mode" in msg
    for k in (-1, 251):
        rc, msg = batch(*good[:3], [1, 0, k], good[4])
        assert rc == _lib.ERR_ARG and "alignment 2: bad max distance" in msg, k
    rc, msg = batch(*good)
    assert rc == valid, msg
    # nothing to do is no fault, with or without a device, whatever the queries hold
    assert batch([b"x"], [], [], [], [], n=0)[0] == _lib.OK
