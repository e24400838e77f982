"""specimux-stats without a GPU: the host aggregator against what the reference's tool printed for the same trace files
(tests/golden/stats/, reference output), and the statistics kernel's per-read code (specimux_amd/csrc/smx_stats_core.h)
run by a CPU simulation against the table the aggregator builds from the oracle's trace of the same reads."""
import json
import os
import random
import subprocess
import sys

import pytest

import stats_utils as U
from oracle import specimux_oracle as O
from parity_utils import make_args, reads_from_set
from stats_utils import CASES, REPO, STATS_GOLDEN, oracle_table, panel_view, parse_sim, queries_of, sim_input, unpack_trace

GOLDEN = os.path.join(REPO, "tests", "golden", "integration_test_suite")


def run_main(argv, capsys):
    from specimux_amd import cli
    rc = cli.trace_main(argv)
    cap = capsys.readouterr()
    return rc, cap.out, cap.err


# ------------------------------------------------------------------ the host aggregator vs the reference's output
@pytest.mark.parametrize("case", CASES)
def test_reports_equal_reference(case, tmp_path, capsys):
    trace = unpack_trace(case, tmp_path)
    for q in queries_of(case):
        if q["kind"] == "sankey":
            out = tmp_path / (q["name"] + ".json")
            rc, _o, err = run_main([trace] + q["args"] + ["--output", str(out)], capsys)
            assert rc == 0, err
            got = json.load(open(out))
            exp = json.load(open(os.path.join(STATS_GOLDEN, case, q["name"] + ".json")))
            exp["links"].sort(key=lambda link: (link["source"], link["target"]))   # the one deliberate difference
            assert got == exp, q["name"]
            assert list(got) == list(exp)
        else:
            rc, text, err = run_main([trace] + q["args"], capsys)
            assert rc == 0, err
            assert text == open(os.path.join(STATS_GOLDEN, case, q["name"] + ".txt"), encoding="utf-8").read(), q["name"]


def test_hierarchical_output_file_and_module_entry(tmp_path):
    trace = unpack_trace("golden_default", tmp_path)
    out = tmp_path / "h.txt"
    res = subprocess.run([sys.executable, "-m", "specimux_amd.trace_stats", trace, "--hierarchical", "pool", "primer_pair",
                          "outcome_detailed", "-o", str(out)], cwd=REPO, capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout == "", res.stderr
    exp = open(os.path.join(STATS_GOLDEN, "golden_default", "hier_pool_pair_detailed.txt"), encoding="utf-8").read()
    assert out.read_text(encoding="utf-8") + "\n" == exp   # the reference prints the text with a newline, writes it without


def test_rejections(tmp_path, capsys):
    trace = unpack_trace("golden_default", tmp_path)
    rc, out, err = run_main([trace, "--hierarchical", "pool", "bogus"], capsys)
    exp = open(os.path.join(STATS_GOLDEN, "golden_default", "invalid_dimension.stderr.txt")).read().strip()
    assert rc == 1 and out == "" and exp in err and exp.startswith("ERROR - Error: Invalid dimensions: ['bogus']. Available: [")
    with pytest.raises(SystemExit) as e:
        run_main([trace, "--hierarchical", "pool", "--count-by", "reads"], capsys)
    assert e.value.code == 2 and "invalid choice: 'reads'" in capsys.readouterr().err
    for dim in ("candidate_match_id", "sequence_id"):   # listed, but a table of counts cannot group by them
        rc, out, err = run_main([trace, "--hierarchical", "pool", dim], capsys)
        assert rc == 1 and out == "" and "cannot be grouped by" in err and dim in err
    rc, out, err = run_main([trace, "--sankey-data", "pool", "outcome"], capsys)
    assert rc == 1 and "--output required for --sankey-data" in err
    rc, out, err = run_main([str(tmp_path / "empty"), "--list-dimensions"], capsys)
    assert rc == 1 and "No trace files found" in err
    with pytest.raises(SystemExit):                        # exactly one report, exactly one source
        run_main([trace, "--hierarchical", "pool", "--list-dimensions"], capsys)
    with pytest.raises(SystemExit):
        run_main([trace, "--table", "x.json", "--list-dimensions"], capsys)
    capsys.readouterr()


def test_save_table_round_trip(tmp_path, capsys):
    from specimux_amd import trace_stats
    trace = unpack_trace("c2_synth", tmp_path)
    saved = tmp_path / "table.json"
    rc, first, err = run_main([trace, "--save-table", str(saved), "--hierarchical", "pool", "primer_pair", "outcome"], capsys)
    assert rc == 0, err
    assert trace_stats.StatsTable.load(saved) == trace_stats.table_from_trace_dir(trace)
    for q in queries_of("c2_synth"):
        if q["kind"] != "sankey":
            rc, text, err = run_main(["--table", str(saved)] + q["args"], capsys)
            assert rc == 0, err
            assert text == open(os.path.join(STATS_GOLDEN, "c2_synth", q["name"] + ".txt"), encoding="utf-8").read()
    rc, _o, err = run_main(["--table", os.path.join(STATS_GOLDEN, "queries.json"), "--list-dimensions"], capsys)
    assert rc == 1


def test_from_run_refuses_several_ranks(monkeypatch, capsys):
    monkeypatch.setenv("WORLD_SIZE", "2")
    rc, out, err = run_main(["--from-run", f"{GOLDEN}/primers.fasta", f"{GOLDEN}/specimens.txt", f"{GOLDEN}/sequences.fastq",
                             "--hierarchical", "pool"], capsys)
    assert rc == 1 and out == "" and "WORLD_SIZE=2" in err and "single process" in err


# ------------------------------------------------------------------ the kernel's per-read code on the CPU
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("stats") / "stats_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "specimux_amd", "csrc"), "-I",
                           os.path.join(REPO, "include"), "-o", exe, os.path.join(REPO, "tests", "cpu", "stats_sim.cpp")])
    return exe


def oracle_setup(pf, sf, **flags):
    a = make_args(**flags)
    opanel = O.load_panel(pf, sf)
    opar = O.setup_params(opanel, search_len=a.search_len, index_edit_distance=a.index_edit_distance,
                          primer_edit_distance=a.primer_edit_distance, preorient=not a.disable_preorient,
                          prefilter=not a.disable_prefilter, trim=a.trim, dereplicate=a.dereplicate,
                          min_length=a.min_length, max_length=a.max_length)
    return a, opanel, opar


def host_replayer(pf, sf, args, view):
    """trace_stats.HostReplay over the product's own panel objects (no device: the hit records come from the caller)."""
    import types
    import specimux_amd as sa
    from specimux_amd import trace_stats
    specimens = sa.read_specimen_file(sf, sa.read_primers_file(pf))
    specimens.validate()
    parameters = sa.setup_match_parameters(args, specimens)
    primers = list(specimens._primers.values())
    assert [p.name for p in primers] == view.primer_names
    panel = types.SimpleNamespace(primers=primers, primer_names=view.primer_names, barcodes=view.barcodes, pools=view.pools,
                                  pairs=view.pairs)
    return trace_stats.HostReplay(panel, parameters, specimens, args, not args.disable_prefilter)


def simulate(sim, tmp_path, pf, sf, reads, flags, capacity=1 << 14, grid=3):
    """-> (table from the simulated kernel code + host-replayed reads, oracle's table, counters, trace rows)."""
    from specimux_amd import trace_stats
    args, opanel, opar = oracle_setup(pf, sf, **flags)
    view = panel_view(opanel)
    blob, _ops, hits, bdist = sim_input(view, opanel, opar, reads)
    path = tmp_path / "sim.bin"
    path.write_bytes(blob)
    res = subprocess.run([sim, os.fspath(path), str(capacity), str(grid)], capture_output=True, text=True)
    if res.returncode != 0:
        return None, None, res, None
    counters, fallback, keys = parse_sim(res.stdout)
    table = trace_stats.table_from_keys(view, list(keys), list(keys.values()))
    if fallback:
        replay = host_replayer(pf, sf, args, view)
        for i in fallback:
            for key in replay.keys_of_read(reads[i][1], hits[i], bdist[i]):
                table.add(*trace_stats.decode_key(view, key))
            table.host_replayed += 1
    exp, rows = oracle_table(opanel, opar, reads)
    assert counters["keys"] == len(keys) and counters["trim_empty"] == len(fallback)
    assert table.host_replayed <= len({r[2] for r in rows if r[3] == "SEQUENCE_TRIM_EMPTY"})
    return table, exp, counters, rows


def assert_tables_equal(got, exp, label):
    if got != exp:
        diff = {k: (got.counts.get(k, 0), exp.counts.get(k, 0)) for k in set(got.counts) | set(exp.counts)
                if got.counts.get(k, 0) != exp.counts.get(k, 0)}
        raise AssertionError(f"{label}: {len(diff)} row(s) differ (kernel code, oracle trace): {list(diff.items())[:6]}")
    assert got.total("sequences") == exp.total("sequences")


SIM_FLAGS = [dict(), dict(dereplicate="none"), dict(trim="tails", disable_preorient=True), dict(min_length=500, max_length=800),
             dict(index_edit_distance=4, disable_prefilter=True)]
_IDS = ["default", "derep-none", "tails-nopreorient", "length-500-800", "e4-noprefilter"]


def synth_reads(which, n=1500):
    from specimux_amd import synth
    pan, seed, kw = {"c1": (synth.panel_c1(), 1001, {}), "c2": (synth.panel_c2(), 2002, {}),
                     "c3": (synth.panel_c3(), 3003, dict(insert_mean=900, insert_sd=250))}[which]
    rs = synth.make_reads(pan, n, seed, windows_only=False, **kw)
    return pan, reads_from_set(rs, range(n), 80)


@pytest.fixture(scope="module", params=["c1", "c2", "c3"])
def synth_case(request, tmp_path_factory):
    pan, reads = synth_reads(request.param)
    pf, sf = pan.write(os.fspath(tmp_path_factory.mktemp(request.param)))
    return request.param, pf, sf, reads


@pytest.mark.parametrize("flags", SIM_FLAGS[:4], ids=_IDS[:4])
def test_sim_golden_reads(sim, tmp_path, flags):
    reads, _ = O.read_sequences(f"{GOLDEN}/sequences.fastq")
    got, exp, counters, _rows = simulate(sim, tmp_path, f"{GOLDEN}/primers.fasta", f"{GOLDEN}/specimens.txt", reads, flags)
    assert_tables_equal(got, exp, f"golden {flags}")
    assert counters["reads"] == 40
    if "min_length" in flags:      # most of the 40 reads are shorter than 500 nt
        assert counters["filtered"] >= 10 and counters["candidates"] >= 10
    else:
        assert counters["candidates"] >= 90 and counters["keys"] >= 12 and counters["discarded"] >= 20


# Floors of the coverage counters per 1 500 synthetic reads.  They say what the inputs must contain for the comparison to
# mean something -- every read a candidate, hundreds of distinct rows on the 768-specimen grids, discarded candidates
# (plentiful on c3, whose pools share a reverse primer), reads with several records where the flags allow them, reads
# whose primary record trimmed to nothing, filtered reads under the length window -- and sit at a half to a third of the
# counts these seeds give, so that a change of the read generator shows up here and not as silence.
@pytest.mark.parametrize("flags", SIM_FLAGS, ids=_IDS)
def test_sim_synthetic_reads(sim, tmp_path, synth_case, flags):
    which, pf, sf, reads = synth_case
    got, exp, c, rows = simulate(sim, tmp_path, pf, sf, reads, flags)
    print(which, flags, c)
    assert_tables_equal(got, exp, f"{which} {flags}")
    assert c["reads"] == 1500
    if "min_length" in flags:
        assert c["filtered"] >= 400 and c["candidates"] >= 500 and c["discarded"] >= (150 if which == "c3" else 10)
        assert c["keys"] >= (15 if which == "c1" else 150)
        return
    assert c["filtered"] == 0 and c["candidates"] >= 1500 and c["trim_empty"] >= 1
    assert got.host_replayed == c["trim_empty"]
    assert c["keys"] >= (10 if which == "c1" else 300)
    assert c["discarded"] >= (800 if which == "c3" else 20)
    if flags.get("index_edit_distance") == 4 and which != "c1":
        assert c["multi_record"] >= (8 if which == "c3" else 3)
    if flags.get("dereplicate") == "none" and which == "c3":
        assert c["multi_record"] >= 4


def test_sim_table_overflow_is_loud(sim, tmp_path):
    pan, reads = synth_reads("c2", 300)
    pf, sf = pan.write(os.fspath(tmp_path / "c2"))
    _g, _e, res, _r = simulate(sim, tmp_path, pf, sf, reads, {}, capacity=8)
    assert res.returncode == 4 and res.stdout.startswith("SMX_ERR_OVERFLOW") and "key " not in res.stdout


def test_sim_local_table_spill(tmp_path, synth_case):
    """The simulation built with a 64-slot local table and 2 probes: most rows find their stretch of it taken and go to
    the global table directly, and the result is the same for any number of workgroups."""
    which, pf, sf, reads = synth_case
    small = os.fspath(tmp_path / "stats_sim_small")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DSTATS_LCAP=64", "-DSTATS_LPROBE=2", "-I",
                           os.path.join(REPO, "specimux_amd", "csrc"), "-I", os.path.join(REPO, "include"), "-o", small,
                           os.path.join(REPO, "tests", "cpu", "stats_sim.cpp")])
    got, exp, c, _rows = simulate(small, tmp_path, pf, sf, reads[:600], {}, grid=1)
    assert_tables_equal(got, exp, which)
    assert c["local_spill"] >= (1 if which == "c1" else 100)
    got7, _e, _c, _r = simulate(small, tmp_path, pf, sf, reads[:600], {}, grid=7)
    assert got7 == got


def test_resolved_record_behind_a_dereplicated_one(sim, tmp_path):
    """The argument behind "resolution = the primary record's rtype, DEREP_FULL read as unknown": two pools share the reverse
    primer; the head window holds barcode A + the first forward primer, then barcode B + the second one; (A, reverse
    barcode) is a specimen, (B, reverse barcode) is not.  The oracle emits a dereplicated full record first and a resolved
    one behind it -- which must be `unknown`, or the kernel would need the extra records."""
    A, B, R, R2 = "ATGCTAGACATCG", "ATAATATTCGGCA", "GCAATAAGGAGCG", "AACGGCCTTGAGG"
    its4, its1f, gits7 = "TCCTCCGCTTATTGATATGC", "CTTGGTCATTTAGAGGAAGTAA", "GTGARTCATCGARTCTTTG"
    pf, sf = tmp_path / "primers.fasta", tmp_path / "specimens.txt"
    pf.write_text(f">ITS4 pool=ITS,ITS2 position=reverse\n{its4}\n>ITS1F pool=ITS position=forward\n{its1f}\n"
                  f">gITS7 pool=ITS2 position=forward\n{gits7}\n")
    sf.write_text("SampleID\tPrimerPool\tFwIndex\tFwPrimer\tRvIndex\tRvPrimer\n"
                  f"S1\tITS\t{A}\tITS1F\t{R}\tITS4\nS2\tITS2\t{B}\tgITS7\t{R2}\tITS4\n")
    rng = random.Random(5)
    insert = "".join(rng.choice("ACGT") for _ in range(420))
    seq = A + its1f + B + gits7.replace("R", "A") + insert + O.revcomp(its4) + O.revcomp(R)
    reads = [("nested", seq, "I" * len(seq)), ("nested_rc", O.revcomp(seq), "I" * len(seq))]
    pf, sf = os.fspath(pf), os.fspath(sf)
    _a, opanel, opar = oracle_setup(pf, sf)
    ops, _t, _m = O.process_sequences(reads, opar, opanel)
    assert [(op.seq_id, op.rtype) for op in ops] == [("nested", O.R_DEREP), ("nested", O.R_UNKNOWN),
                                                     ("nested_rc", O.R_DEREP), ("nested_rc", O.R_UNKNOWN)]
    got, exp, counters, rows = simulate(sim, tmp_path, pf, sf, reads, {})
    assert_tables_equal(got, exp, "nested")
    assert counters["multi_record"] == 2 and counters["candidates"] == 4
    assert [r[5] for r in rows if r[3] == "SPECIMEN_RESOLVED"] == ["unknown", "unknown"]
    assert {row[7:9] for (row, _f) in exp.counts} == {("unknown", "unknown")}


# ------------------------------------------------------------------ synthetic hit tables: the reference against the twin
# The cases of tests/test_stats_kernel_gpu.py (stats_utils.case_*), run through the simulation: its table must equal
# stats_utils.rows_reference, its fallback list the reference's, for one workgroup and for seven.  `local_spill` proves
# here, where it can be counted, that the inputs built to pass the workgroup's table by do so.
@pytest.fixture(scope="module")
def sim_small(tmp_path_factory):
    exe = os.fspath(tmp_path_factory.mktemp("stats_small") / "stats_sim_small")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DSTATS_LCAP=64", "-DSTATS_LPROBE=2", "-I",
                           os.path.join(REPO, "specimux_amd", "csrc"), "-I", os.path.join(REPO, "include"), "-o", exe,
                           os.path.join(REPO, "tests", "cpu", "stats_sim.cpp")])
    return exe


@pytest.fixture(scope="module")
def facts(tmp_path_factory):
    """{c2, c3, c9: (NP, pdir, pairs, number of barcodes)} from the oracle's panel; c9 = stats_utils.panel_nine_pairs."""
    from specimux_amd import synth
    out = {}
    for name, pan in (("c2", synth.panel_c2()), ("c3", synth.panel_c3()), ("c9", U.panel_nine_pairs())):
        pf, sf = pan.write(os.fspath(tmp_path_factory.mktemp("facts_" + name)))
        view = panel_view(O.load_panel(pf, sf))
        out[name] = (len(view.primers), view.pdir, view.pairs, len(view.barcodes))
    assert out["c2"][0] == 2 and out["c3"][0] == out["c9"][0] == 8 and len(out["c3"][2]) == 4 and len(out["c9"][2]) == 9
    return out


def run_twin(exe, tmp_path, fact, preorient, hits, ops, capacity, grid):
    NP, pdir, pairs, _nb = fact
    path = tmp_path / "synthetic.bin"
    path.write_bytes(U.sim_bytes(NP, pdir, pairs, preorient, hits, ops))
    return subprocess.run([exe, os.fspath(path), str(capacity), str(grid)], capture_output=True, text=True)


def twin_equals_reference(exe, tmp_path, fact, preorient, hits, ops, capacity=1 << 14, grids=(1, 7), want=None):
    """-> (the simulation's counters per grid, the reference's table and fallback list)"""
    NP, pdir, pairs, _nb = fact
    table, fallback = want or U.rows_reference(NP, pdir, pairs, preorient, hits, ops)
    out = []
    for grid in grids:
        res = run_twin(exe, tmp_path, fact, preorient, hits, ops, capacity, grid)
        assert res.returncode == 0, res.stdout[:300] + res.stderr[:300]
        counters, got_fallback, got = parse_sim(res.stdout)
        assert got == dict(table), (grid, len(got), len(table), [(hex(k), got.get(k), table.get(k)) for k in set(got) ^ set(table)][:5])
        assert sorted(got_fallback) == fallback and counters["reads"] == len(ops)
        out.append(counters)
    return out, table, fallback


@pytest.fixture(scope="module")
def truth_table():
    return U.case_truth_table()


@pytest.fixture(scope="module")
def random_case(facts):
    NP, pdir, pairs, nb = facts["c9"]
    hits, ops = U.case_random(NP, nb - 1)
    return hits, ops, {pre: U.rows_per_read(NP, pdir, pairs, pre, hits, ops) for pre in (True, False)}


@pytest.mark.parametrize("preorient", [True, False])
def test_twin_truth_table(sim, tmp_path, facts, truth_table, preorient):
    hits, ops = truth_table
    _c, table, fallback = twin_equals_reference(sim, tmp_path, facts["c2"], preorient, hits, ops)
    U.assert_truth_table_coverage(table, fallback, ops, preorient)


@pytest.mark.parametrize("preorient", [True, False])
def test_twin_random_hits(sim, sim_small, tmp_path, facts, random_case, preorient):
    hits, ops, _rows = random_case
    counters, table, _fb = twin_equals_reference(sim, tmp_path, facts["c9"], preorient, hits, ops)
    assert len(table) >= U.LCAP + 1                          # more keys than one workgroup's table has slots
    assert all(c["local_spill"] > 0 for c in counters)
    small, _t, _f = twin_equals_reference(sim_small, tmp_path, facts["c9"], preorient, hits, ops)
    assert all(c["local_spill"] > 10000 for c in small)


@pytest.mark.parametrize("uses", ["1+j%6", "8x256", "48x256"])
def test_twin_local_bypass_and_wrap(sim, sim_small, tmp_path, facts, uses):
    NP, _pdir, pairs, _nb = facts["c3"]
    hits, ops, _keys = U.case_bypass(NP, pairs[0], 1, U.BYPASS_USES[uses], 71)
    for exe in (sim, sim_small):
        counters, table, _fb = twin_equals_reference(exe, tmp_path, facts["c3"], True, hits, ops, capacity=64)
        assert len(table) == 40 and sum(table.values()) == len(ops)
        # a workgroup that sees them all holds at most a probe run of these keys: the other 24 (38 in the small build) pass
        # it by every time
        floor = sum(sorted(table.values())[:40 - (U.LPROBE if exe == sim else 2)])
        assert counters[0]["local_spill"] >= floor >= 24 and counters[1]["local_spill"] >= 24


def test_twin_global_table_exactly_full_and_one_too_many(sim, sim_small, tmp_path, facts):
    NP, _pdir, pairs, _nb = facts["c3"]
    hits, ops = U.case_full_table(NP, pairs[0], 1, 8)
    for exe in (sim, sim_small):
        counters, table, _fb = twin_equals_reference(exe, tmp_path, facts["c3"], True, hits, ops, capacity=8)
        assert sorted(table.values()) == [5] * 8
        # eight keys never exhaust the stock table's 16 probes: only the 2-probe build drives these past the local table
        assert all((c["local_spill"] > 0) == (exe == sim_small) for c in counters)
    hits, ops = U.case_full_table(NP, pairs[0], 1, 9)
    for exe in (sim, sim_small):
        for grid in (1, 7):
            res = run_twin(exe, tmp_path, facts["c3"], True, hits, ops, 8, grid)
            assert res.returncode == 4 and res.stdout.startswith("SMX_ERR_OVERFLOW") and "key " not in res.stdout
            assert "(8 slots) is full: 5 increments found no slot" in res.stdout


def test_twin_grid_stride_with_a_remainder(sim, tmp_path, facts, random_case):
    NP, pdir, pairs, _nb = facts["c9"]
    hits_b, ops_b, rows_b = random_case
    G = 3
    hits, ops, use, pool = U.case_stride(hits_b, ops_b, rows_b[True], G)
    want = U.reference_of_templates(rows_b[True], pool, use)
    assert len(ops) == 2 * G * 256 + 77 and want == U.rows_reference(NP, pdir, pairs, True, hits, ops)
    twin_equals_reference(sim, tmp_path, facts["c9"], True, hits, ops, grids=(G,), want=want)


def test_twin_fallback_list(sim, tmp_path, facts):
    hits, ops = U.case_fallback()
    _c, table, fallback = twin_equals_reference(sim, tmp_path, facts["c2"], True, hits, ops)
    assert 600 <= len(fallback) <= 800


def test_twin_field_edges(sim, tmp_path, facts):
    NP, _pdir, pairs, _nb = facts["c3"]
    hits, ops = U.case_field_edges(NP, pairs)
    _c, table, _fb = twin_equals_reference(sim, tmp_path, facts["c3"], True, hits, ops)
    U.assert_field_edges(table, len(pairs))
