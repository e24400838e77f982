"""CPU side of the scorer-case tests (no GPU needed): the census that keeps tests/test_scorer_cases_gpu.py honest, the panel
compiler's flattening of the hand-written panels, and hand-derived anchors for the oracle's restatements of the specimen
lookups and the dereplication (oracle/specimux_oracle.py: _resolve, get_paired, specimen_for_exact, specimens_for,
dereplicate, derep_partial, resolve_specimen).

Those restatements were re-read against the reference lines they cite for wildcards, duplicate rows, a shared primer
sequence and a None group that holds full candidates (databases.py:135-167, :197-264; demultiplex.py:262-393, :396-477,
:541-598; models.py:20-31 -- PrimerInfo defines no __eq__, so `p1 in p1s` is object identity).  No divergence was found;
the anchors below pin the cases that were read."""
import os

import pytest

import scorer_utils as SU
from oracle import specimux_oracle as O
from parity_utils import Both

# What cannot occur, per flag set (it holds for every panel): the reason is in the reference's control flow, not in the reads.
#   multiple_untied  MULTIPLE_SPECIMENS is only produced by resolve_specimen's full branch (demultiplex.py:558-564); with
#                    --dereplicate best a full candidate reaches resolve_specimen only through the None group, i.e. when
#                    specimen_for_exact found nothing for any tied combination, and then specimens_for finds nothing either.
#   cand_twice       with --dereplicate none every best candidate is resolved and written exactly once (:181-197).
# Every other situation and property can occur on every one of the five panels: two candidates need either two primer
# pairs that match one read (multi, two_pairs, wide: W8 / W9; same_sequence and one_pair_sparse have one pair) or an
# undecided orientation vote, which the both-ends and dual read families give on every panel.
CANNOT = {"best": {"multiple_untied"}, "none": {"cand_twice"}}


@pytest.fixture(scope="module")
def panel_files(tmp_path_factory):
    out = {}
    for name, pan in SU.PANELS.items():
        out[name] = pan.write(os.fspath(tmp_path_factory.mktemp(name)))
    return out


def test_barcodes_keep_k_idx_3_and_tie_as_designed():
    """The hand-built barcodes: F1, F2 (R1, R2) at Hamming distance 6 from F0 (R0) and from each other, every pair of the
    12 at edit distance >= 5 in the frame setup_match_parameters compares them in, so k_idx stays 3."""
    import itertools
    from oracle import edlib_semantics as E
    for B, three, two in ((SU.F, SU.F3WAY, SU.F2WAY), (SU.R, SU.R3WAY, SU.R2WAY)):
        ham = lambda a, b: sum(x != y for x, y in zip(a, b))   # noqa: E731
        assert [ham(a, b) for a, b in itertools.combinations(B[:3], 2)] == [6, 6, 6]
        assert [ham(three, b) for b in B[:3]] == [3, 3, 3] and [ham(two, b) for b in B[:2]] == [3, 3]
        assert all(len(b) == 13 for b in B)
    comb = SU.F + [O.revcomp(b) for b in SU.R]
    assert min(E.align(a, b, E.NW, -1, iupac=False)["editDistance"] for a, b in itertools.combinations(comb, 2)) == 5


@pytest.mark.parametrize("name", list(SU.PANELS))
def test_census(panel_files, name):
    """Every situation and property that can occur has at least 8 constructed reads, on every flag set: the condition
    that keeps the GPU comparison from passing on an input that misses a scorer branch.  Oracle only."""
    pf, sf = panel_files[name]
    reads = SU.make_reads(SU.PANELS[name])
    assert 400 <= len(reads) <= 660
    assert sum(1 for r in reads if 30 <= len(r[1]) <= 79) >= 8
    for fname, flags in SU.FLAG_SETS.items():
        panel, par = SU.oracle_setup(pf, sf, **flags)
        assert par.max_dist_index == flags.get("index_edit_distance", 3)
        counts, _labels = SU.census(par, panel, reads)
        cannot = CANNOT[par.dereplicate]
        print(f"{name} {fname}: " + ", ".join(f"{k} {counts[k]}" for k in SU.SITUATIONS + SU.PROPERTIES))
        assert set(counts) <= set(SU.SITUATIONS + SU.PROPERTIES), set(counts) - set(SU.SITUATIONS + SU.PROPERTIES)
        for k in SU.SITUATIONS + SU.PROPERTIES:
            if k in cannot:
                assert counts[k] == 0, (name, fname, k, counts[k])
            else:
                assert counts[k] >= SU.MIN_READS, (name, fname, k, counts[k])


def _compiled(pf, sf, **flags):
    from specimux_amd.demultiplex import compiled_panel
    both = Both(pf, sf, **flags)
    return both, compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)


def _bc_lists(cp):
    off, flat = cp._keep["primer_bc_off"], cp._keep["primer_bc"]
    return [[cp.barcodes[int(i)] for i in flat[int(off[p]):int(off[p + 1])]] for p in range(len(cp.primers))]


def test_flattening_multi(panel_files):
    both, cp = _compiled(*panel_files["multi"])
    F, R = SU.F, SU.R
    # registration order (Q5): FA1, RA1 (row 1), FA2 (the * of row 3), RA2 (the * of row 4), FB (row 12)
    assert cp.primer_names == ["FA1", "RA1", "FA2", "RA2", "FB"]
    A, B = cp.pools.index("A"), cp.pools.index("B")
    assert cp.pairs == [(0, 1, A), (0, 3, A), (2, 1, A), (2, 3, A), (4, 1, B)]     # FB shares no specimen with RA2
    fa1, ra1, fa2, ra2, fb = 1, 2, 4, 8, 16
    assert list(cp._keep["spec_p1mask"]) == [fa1, fa1, fa1 | fa2, fa2, fa1 | fa2, fa1, fa1, fa1, fa1, fa1, fa2, fb, fb, fa1, fa1]
    assert list(cp._keep["spec_p2mask"]) == [ra1, ra1, ra1, ra1 | ra2, ra1 | ra2, ra2, ra1, ra1, ra1, ra1, ra2, ra1, ra1, ra1, ra1]
    assert [cp.pools[i] for i in cp._keep["spec_pool"]] == ["A"] * 11 + ["B", "B", "A", "A"]
    assert cp.barcodes == F + R
    assert _bc_lists(cp) == [F, R, [F[0], F[1], F[2], F[4]], [R[1], R[2], R[4]], [F[3], F[4]]]
    assert [cp.barcodes[i] for i in cp._keep["spec_b1"]][:5] == [F[0], F[1], F[0], F[1], F[2]]
    assert cp.counts_len == 8 + 15 and cp.hits_per_read == 10 and both.parameters.max_dist_index == 3
    assert list(cp._keep["primer_k"]) == [7, 6, 7, 6, 5] and list(cp._keep["primer_file_index"]) == [0, 2, 1, 3, 4]


def test_flattening_wide(panel_files):
    """36 primer pairs, 72 candidates: more than the 64 bits of the scorer's candidate mask; the library takes the panel."""
    both, cp = _compiled(*panel_files["wide"])
    F, R = SU.F, SU.R
    assert cp.primer_names == [f"W{i}" for i in range(1, 10)] + [f"X{i}" for i in range(1, 5)]   # row 1 is * / *
    assert cp.pairs == [(i, 9 + j, 0) for i in range(9) for j in range(4)] and cp.pools == ["W"]
    allf, allr = 0x1FF, 0xF << 9
    w = lambda i: 1 << (i - 1)      # noqa: E731
    x = lambda i: 1 << (8 + i)      # noqa: E731
    assert list(cp._keep["spec_p1mask"]) == [allf, w(8), w(9), allf, allf, w(8), w(1), w(9), w(9), w(8), w(5), allf, w(1), w(1)]
    assert list(cp._keep["spec_p2mask"]) == [allr, allr, x(4), x(1), allr, x(4), x(1), x(4), x(4), allr, x(2), allr, x(1), allr]
    bl = dict(zip(cp.primer_names, _bc_lists(cp)))
    assert bl["W1"] == [F[0], F[1], F[2], F[3]] and bl["W8"] == [F[0], F[1], F[2], F[4]] and bl["W9"] == [F[0], F[1], F[2], F[3]]
    assert bl["W5"] == [F[0], F[1], F[2], F[5]] and bl["W2"] == [F[0], F[1], F[2]]
    assert bl["X1"] == R[:5] and bl["X4"] == R[:5] and bl["X2"] == [R[0], R[2], R[4], R[5], R[1]] and bl["X3"] == [R[0], R[2], R[4], R[1]]
    assert cp.counts_len == 8 + 14 and cp.hits_per_read == 26


def test_flattening_same_sequence(panel_files):
    """One sequence under two names (Q5): the name registered first (FA1, row 1) serves the sequence and takes the barcodes
    and specimens of both; a row that names the other one has a zero p1 mask -- it can never be matched -- while a
    wildcard row, which holds both objects, keeps its bit."""
    both, cp = _compiled(*panel_files["same_sequence"])
    F, R = SU.F, SU.R
    assert cp.primer_names == ["FA1", "RA1"] and cp.pairs == [(0, 1, 0)]
    rows = SU.PANELS["same_sequence"].rows
    assert list(cp._keep["spec_p1mask"]) == [0 if r[3] == "FA1B" else 1 for r in rows]
    assert list(cp._keep["spec_p1mask"]) == [1, 0, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1]
    assert list(cp._keep["spec_p2mask"]) == [2] * 12
    assert _bc_lists(cp) == [F, R]       # FA1 carries F1 (row 2), F3 (row 6) and F5 (row 10) from FA1B's rows
    assert cp.specimen_ids == [r[0] for r in rows]


def test_oracle_lookups_on_wildcards_duplicates_and_shared_sequence(panel_files):
    """Hand-derived from the sheets (scorer_utils) and databases.py:219-245."""
    F, R = SU.F, SU.R
    pan = O.load_panel(*panel_files["multi"])
    p = pan.by_name
    assert pan.specimen_for_exact(F[0], R[1], p["FA2"], p["RA1"]) == "s03"          # * expanded to FA1 and FA2
    assert pan.specimen_for_exact(F[1], R[1], p["FA1"], p["RA1"]) is None           # row 4 names FA2 only
    assert pan.specimen_for_exact(F[1], R[1], p["FA2"], p["RA2"]) == "s04"
    assert pan.specimen_for_exact(F[2], R[2], p["FA2"], p["RA2"]) == "s05"          # - / -
    assert pan.specimen_for_exact(F[3], R[3], p["FA1"], p["RA1"]) == "s08"          # first of two ids
    assert pan.specimens_for([F[3]], [R[3]], p["FA1"], p["RA1"]) == ["s08", "s09"]  # MULTIPLE from an untied pair
    assert pan.specimens_for([F[3]], [R[3]], p["FB"], p["RA1"]) == ["s12"] and pan.specimen_pool("s12") == "B"
    assert pan.specimens_for([F[4]], [R[4]], p["FA2"], p["RA2"]) == ["s11"]         # the same pair under other primers
    assert pan.specimens_for(F[:3], R[:2], p["FA1"], p["RA1"]) == ["s01", "s02", "s03", "s07", "s15"]
    assert [x.name for x in pan.get_paired(SU.FA1)] == ["RA1", "RA2"] and [x.name for x in pan.get_paired(SU.FB)] == ["RA1"]
    same = O.load_panel(*panel_files["same_sequence"])
    q = same.by_name
    assert list(same.primers) == [SU.FA1, SU.RA1] and same.primers[SU.FA1] is q["FA1"]
    assert same.specimen_for_exact(F[1], R[0], q["FA1"], q["RA1"]) == "s11"         # row 2 (FA1B) is skipped
    assert same.specimen_for_exact(F[3], R[3], q["FA1"], q["RA1"]) == "s07"
    assert same.specimen_for_exact(F[5], R[5], q["FA1"], q["RA1"]) is None          # named by an FA1B row only
    assert same.specimen_for_exact(F[2], R[2], q["FA1"], q["RA1"]) == "s04"         # the * row holds FA1 too
    assert same.specimens_for([F[4]], [R[4]], q["FA1"], q["RA1"]) == ["s08", "s12"]


def test_oracle_none_group_holds_full_candidates(panel_files):
    """dereplicate_matches with a None group of full candidates (demultiplex.py:331-365), by hand.  The read carries F1,
    FA1, RA1, R1 on the `multi` panel: four full candidates in pair order (FA1, RA1), (FA1, RA2), (FA2, RA1), (FA2, RA2).
    Only row 4 (F1, FA2, R1, *) holds (F1, R1): the first two candidates map to nothing, the last two to s04.  Groups in
    first-appearance order: None, then s04.  The None group writes both its members as unknown, in order, before s04;
    s04's winner is (FA2, RA1): primer distances 2 + 0 against 2 + 2."""
    pf, sf = panel_files["multi"]
    panel, par = SU.oracle_setup(pf, sf)
    s = SU._structure("b1", SU.FA1, "b1", SU.RA1)
    ops, total, matched = O.process_sequences([("r", s, "I" * len(s))], par, panel)
    assert [(op.sample_id, op.p1, op.p2, op.code, op.rtype, op.pool) for op in ops] == [
        ("unknown", "FA1", "RA1", "0,0,0,0", O.R_UNKNOWN, "A"), ("unknown", "FA1", "RA2", "0,0,0,2", O.R_UNKNOWN, "A"),
        ("s04", "FA2", "RA1", "2,0,0,0", O.R_DEREP, "A")]
    assert (total, matched) == (1, 1)
    # trim barcodes, Q8: each candidate is written once here, so every record has the same extent
    assert len({op.sequence for op in ops}) == 1
    # --dereplicate none: the four candidates in order, resolve_specimen each
    panel, par = SU.oracle_setup(pf, sf, dereplicate="none")
    ops, _t, matched = O.process_sequences([("r", s, "I" * len(s))], par, panel)
    assert [(op.sample_id, op.p1, op.p2, op.rtype) for op in ops] == [
        ("unknown", "FA1", "RA1", O.R_UNKNOWN), ("unknown", "FA1", "RA2", O.R_UNKNOWN), ("s04", "FA2", "RA1", O.R_FULL),
        ("s04", "FA2", "RA2", O.R_FULL)]
    assert matched == 1
