"""specimux-barcodes on the GPU: the (flank, count) table and the per-primer counters the count kernel leaves equal a brute
force count in plain Python over the same windows and the hit dump of the same launch; accumulation is independent of the
batch cut and of the reads' strand; the assign kernel agrees with the demux kernel's own barcode search wherever both look
at the same string; and the tool finds the barcodes a sheet withholds."""
import ctypes as C
import gzip
import json
import os
import shutil

import numpy as np
import pytest

from parity_utils import Both, tmp_panel

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "integration_test_suite")
HITS, PRUNED, SHORT_READ, SHORT_FLANK, AMBIGUOUS, COUNTED = range(6)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def lib():
    from specimux_amd import _lib
    lib = _lib.load()
    n = C.c_int(0)
    _lib.check(lib.smx_device_init(0, C.byref(n)))
    assert n.value >= 1
    return lib


def near_panel():
    """c1's primers with four forward barcodes of which the second is the first with one letter changed."""
    from specimux_amd import synth
    f, r = synth.make_barcodes(4, 3, seed=11)
    twin = f[0][:5] + ("A" if f[0][5] != "A" else "C") + f[0][6:]
    return synth.Panel([("ITS", "ITS1F", synth.ITS1F, "ITS4", synth.ITS4)], [f[0], twin, f[2], f[3]], r)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """name -> (Both, CompiledPanel, reads [(id, sequence, quality)]): the reads are generated once and shared."""
    from specimux_amd import synth
    from specimux_amd.demultiplex import compiled_panel
    out = {}
    for name, pan, n, seed, flags, gen in (
            ("c1", synth.panel_c1(), 2500, 31, dict(), dict()),
            ("c3", synth.panel_c3(), 2000, 32, dict(), dict(insert_mean=900, insert_sd=250)),
            ("c1_nopf", synth.panel_c1(), 2500, 33, dict(disable_prefilter=True), dict()),
            ("c3_nopf", synth.panel_c3(), 2000, 34, dict(disable_prefilter=True), dict(insert_mean=900, insert_sd=250)),
            ("near_nopf", near_panel(), 3000, 35, dict(disable_prefilter=True, index_edit_distance=3), dict())):
        pf, sf = tmp_panel(tmp_path_factory, pan, "flank_" + name)
        both = Both(pf, sf, **flags)
        cp = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
        rs = synth.make_reads(pan, n, seed, windows_only=False, **gen)
        out[name] = (both, cp, [(f"r{i}", s, q) for i, (s, q) in enumerate(zip(rs.reads, rs.quals))], pan)
    return out


def windows_of(cp, reads):
    from specimux_amd.demultiplex import concat_records
    from specimux_amd.io_utils import SeqRecord
    bases, offsets, _seqs = concat_records([SeqRecord(s, rid, rid, q) for rid, s, q in reads])
    return cp.pack_windows(bases, offsets)


def cut(windows, lens, sizes):
    """The batch list that walks the reads in batches of sizes[0], sizes[1], ... (cyclically)."""
    out, a, i = [], 0, 0
    while a < len(lens):
        b = min(len(lens), a + sizes[i % len(sizes)])
        out.append((windows[a:b], lens[a:b], None))
        a, i = b, i + 1
    return out


def device_flank(cp, batches, capacity=1 << 16, n_slots=2, want_hits=False):
    """(table {key: count}, counters [NP, 6], hit dump of the launches) of the batches counted on the device."""
    from specimux_amd import _lib, barcodes, trace_stats
    fl = barcodes.DeviceFlank(cp, capacity)
    dumps = []
    H = cp.hits_per_read

    def enqueue(s, sp, n):
        fl.accumulate(sp, s.d_windows.data_ptr(), s.d_lens.data_ptr(), s.d_hits.data_ptr(), n)
        if want_hits:
            raw = s.d_hits[:n * H * _lib.HIT_DTYPE.itemsize].cpu().numpy()
            dumps.append(np.frombuffer(raw.tobytes(), dtype=_lib.HIT_DTYPE).reshape(n, H))
    try:
        trace_stats.stream_batches(cp, batches, enqueue, n_slots=n_slots)
        keys, counts, counters = fl.read()
    finally:
        fl.close()
    return dict(zip(keys.tolist(), counts.tolist())), counters, (np.concatenate(dumps) if dumps else None)


def brute_force(cp, windows, lens, hits):
    """The definitions of include/smx.h ("Barcode survey") in plain Python over strings.  Returns (table, counters, one
    record (read, primer, end, category, key or None) per hit)."""
    S, Lb, k = cp.search_len, int(cp.desc.barcode_len_max), int(cp.desc.k_index)
    W, NP = Lb + k, len(cp.primers)
    table, counters, records = {}, np.zeros((NP, 6), dtype=np.uint64), []
    for i in range(len(lens)):
        L = int(lens[i])
        head, tail = windows[i, :S].tobytes(), windows[i, S:2 * S].tobytes()
        for p in range(NP):
            for e in (0, 1):
                h = hits[i, 2 * p + e]
                if h["pdist"] < 0:
                    continue
                key = None
                if h["bbest"] == -2:
                    cat = PRUNED
                elif L < S:
                    cat = SHORT_READ
                else:
                    # the end string's last S letters: the tail window, or the reverse complement of the head window
                    end_string = tail if e else head[::-1].translate(_COMP)
                    j_end = int(h["first_end"]) - (L - S)
                    assert 0 <= j_end < S
                    flank = end_string[j_end + 1:j_end + 1 + W]
                    if len(flank) < Lb - k:
                        cat = SHORT_FLANK
                    elif any(ch not in b"ACGT" for ch in flank):
                        cat = AMBIGUOUS
                    else:
                        cat = COUNTED
                        key = sum(b"ACGT".index(ch) << (2 * t) for t, ch in enumerate(flank))
                        key |= len(flank) << 52 | int(h["bbest"] >= 0) << 57 | p << 58
                        table[key] = table.get(key, 0) + 1
                counters[p, cat] += 1
                counters[p, HITS] += 1
                records.append((i, p, e, cat, key))
    return table, counters, records


def assert_counter_rules(table, counters):
    for p in range(len(counters)):
        assert int(counters[p, HITS]) == int(counters[p, 1:].sum())
        assert int(counters[p, COUNTED]) == sum(n for key, n in table.items() if key >> 58 == p)


@pytest.mark.parametrize("name", ["c1", "c3"])
def test_table_and_counters_equal_brute_force(lib, cases, name):
    _both, cp, reads, _pan = cases[name]
    windows, lens = windows_of(cp, reads)
    table, counters, hits = device_flank(cp, [(windows, lens, None)], want_hits=True)
    want, want_counters, _records = brute_force(cp, windows, lens, hits)
    assert table == want
    assert np.array_equal(counters, want_counters)
    assert_counter_rules(table, counters)
    print(f"{name}: {int(counters[:, HITS].sum())} hits, {len(table)} distinct flanks, counters {counters.sum(axis=0).tolist()}")
    assert counters[:, COUNTED].sum() > len(reads) and counters[:, SHORT_FLANK].sum() > 0 and counters[:, SHORT_READ].sum() > 0
    assert max(table.values()) > 1 and sum(1 for n in table.values() if n == 1) > len(table) // 2   # repeats and a singleton tail


def test_split_invariance_and_strand(lib, cases):
    from specimux_amd import synth
    _both, cp, reads, _pan = cases["c1"]
    windows, lens = windows_of(cp, reads)
    whole, counters, _h = device_flank(cp, [(windows, lens, None)])
    parts, counters_p, _h = device_flank(cp, cut(windows, lens, [1, 63, 64, 257]), n_slots=3)
    assert parts == whole and np.array_equal(counters, counters_p)
    # every read reverse-complemented: the flipped half of the set becomes the other half
    wr, lr = windows_of(cp, [(rid, synth.revcomp(s), q[::-1]) for rid, s, q in reads])
    flipped, counters_f, _h = device_flank(cp, [(wr, lr, None)])
    assert flipped == whole and np.array_equal(counters, counters_f)


def test_small_table_overflows_loudly(lib, cases):
    from specimux_amd import _lib, barcodes, trace_stats
    _both, cp, reads, _pan = cases["c1"]
    windows, lens = windows_of(cp, reads)
    fl = barcodes.DeviceFlank(cp, 8)
    try:
        trace_stats.stream_batches(cp, [(windows, lens, None)], lambda s, sp, n: fl.accumulate(
            sp, s.d_windows.data_ptr(), s.d_lens.data_ptr(), s.d_hits.data_ptr(), n))
        n, dropped = C.c_uint32(7), C.c_uint64(0)
        rc = lib.smx_flank_read(fl.handle, None, None, 0, C.byref(n), None, C.byref(dropped))
        assert rc == _lib.ERR_OVERFLOW and dropped.value > 0 and n.value == 0
        assert "--table-capacity" in lib.smx_last_error().decode()
        with pytest.raises(_lib.SmxError) as err:
            fl.read()
        assert err.value.code == _lib.ERR_OVERFLOW
    finally:
        fl.close()


def test_forced_paths_land_in_their_counters(lib, cases):
    from specimux_amd import synth
    _both, cp, _reads, pan = cases["c1"]
    rng = np.random.default_rng(5)

    def rand(n):
        return "".join("ACGT"[c] for c in rng.integers(0, 4, n))
    b1, b2 = pan.fwd[0], pan.rev[1]
    p1, p2rc, b2rc = synth.ITS1F, synth.revcomp(synth.ITS4), synth.revcomp(b2)
    insert = rand(400)
    reads = [("plain", rand(11) + b1 + p1 + insert + p2rc + b2rc + rand(9)),
             # search_len - 1 bases: the longest read below search_len, whose whole window is still the primer's target
             ("short", rand(5) + b1 + p1 + rand(39)),
             ("n_in_flank", rand(11) + b1[:6] + "N" + b1[7:] + p1 + insert + p2rc + b2rc + rand(9)),
             ("primer_at_read_start", p1 + insert + p2rc + b2rc + rand(9))]                    # flen = 0 at ITS1F
    reads = [(rid, s, "I" * len(s)) for rid, s in reads]
    windows, lens = windows_of(cp, reads)
    table, counters, hits = device_flank(cp, [(windows, lens, None)], want_hits=True)
    want, want_counters, records = brute_force(cp, windows, lens, hits)
    assert table == want and np.array_equal(counters, want_counters)
    its1f = cp.primer_names.index("ITS1F")
    cats = {reads[i][0]: cat for i, p, _e, cat, _key in records if p == its1f}
    assert cats == {"plain": COUNTED, "short": SHORT_READ, "n_in_flank": AMBIGUOUS, "primer_at_read_start": SHORT_FLANK}
    at_start = next(h for i, p, e, _c, _k in records if p == its1f and reads[i][0] == "primer_at_read_start"
                    for h in [hits[i, 2 * p + e]])
    assert int(at_start["first_end"]) == int(lens[3]) - 1


@pytest.mark.parametrize("name", ["c1_nopf", "c3_nopf", "near_nopf"])
def test_assign_agrees_with_the_demux_kernel(lib, cases, name):
    """A cross-check between two kernels of this project, on hits with one primer location.  The assign kernel's reference
    is the plain twin of tests/test_flank_assign_gpu.py."""
    from specimux_amd import barcodes
    from specimux_amd.models import reverse_complement
    _both, cp, reads, _pan = cases[name]
    k = int(cp.desc.k_index)
    windows, lens = windows_of(cp, reads)
    table, _counters, hits = device_flank(cp, [(windows, lens, None)], want_hits=True)
    want, _c, records = brute_force(cp, windows, lens, hits)
    assert table == want
    cands, global_index = [], []
    for p, primer in enumerate(cp.primers):
        cands += [(p, reverse_complement(b)) for b in primer.barcodes]
        global_index += [cp.barcodes.index(b) for b in primer.barcodes]
    keys = np.array(sorted(table), dtype=np.uint64)
    best, first, ntied = barcodes.assign(keys, cands, k)
    at = {int(key): i for i, key in enumerate(keys)}
    one = many = tied = 0
    for i, p, e, cat, key in records:
        if cat != COUNTED:
            continue
        h, a = hits[i, 2 * p + e], at[key]
        ctx = (reads[i][0], cp.primer_names[p], e, h, int(best[a]), int(first[a]), int(ntied[a]))
        if h["nloc"] == 1:
            one += 1
            assert int(best[a]) == int(h["bbest"]), ctx
            assert (key >> 57 & 1) == int(best[a] >= 0), ctx
            if best[a] >= 0:
                assert global_index[first[a]] == int(h["first_tied"]) and int(ntied[a]) == int(h["ntied"]), ctx
                tied += int(ntied[a]) > 1
            else:
                assert first[a] == -1 and ntied[a] == 0, ctx
        else:
            many += 1
            if best[a] >= 0:
                assert 0 <= int(h["bbest"]) <= int(best[a]), ctx
    print(f"{name}: {one} hits with one primer location, {many} with several, {tied} with tied barcodes")
    assert one > 2000
    if name == "near_nopf":
        assert tied > 0


# ------------------------------------------------------------------------------------------------ the tool
def _run_tool(argv, capsys):
    from specimux_amd import cli
    rc = cli.barcodes_main([os.fspath(a) for a in argv])
    cap = capsys.readouterr()
    assert rc == 0, cap.err
    return cap.out


@pytest.fixture(scope="module")
def discovery(tmp_path_factory):
    """Reads of a 4 x 3 barcode panel, a sheet without the fourth forward and the third reverse barcode, and one that
    lists the fourth forward barcode reverse-complemented."""
    from specimux_amd import synth
    d = tmp_path_factory.mktemp("flank_discovery")
    f, r = synth.make_barcodes(4, 3, seed=7)
    pools = [("ITS", "ITS1F", synth.ITS1F, "ITS4", synth.ITS4)]
    fq = os.fspath(d / "reads.fastq")
    synth.make_reads(synth.Panel(pools, f, r), 3000, 5, windows_only=False).write_fastq(fq)
    withheld = synth.Panel(pools, f[:3], r[:2]).write(os.fspath(d / "withheld"))
    entered_rc = synth.Panel(pools, f[:3] + [synth.revcomp(f[3])], r[:2]).write(os.fspath(d / "entered_rc"))
    return f, r, fq, withheld, entered_rc


def test_discovery_of_withheld_barcodes(lib, discovery, tmp_path, capsys):
    f, r, fq, (pf, sf), (pf2, sf2) = discovery
    out = _run_tool([pf, sf, fq, "--json", tmp_path / "s.json", "--report", tmp_path / "s.tsv", "--top", "5"], capsys)
    doc = json.load(open(tmp_path / "s.json"))
    assert doc["reads"] == 3000 and [p["primer"] for p in doc["primers"]] == ["ITS1F", "ITS4"]
    for prim, listed, missing in zip(doc["primers"], (f[:3], r[:2]), (f[3], r[2])):
        rows = prim["candidates"]
        print(prim["primer"], prim["counters"], "unexplained", prim["unexplained"],
              [(x["barcode"], x["status"], x["exact"], sum(x["support"])) for x in rows[:8]])
        known = [x for x in rows if x["status"] == "known"]
        novel = [x for x in rows if x["status"] == "novel"]
        assert [x["barcode"] for x in known] == list(listed) and all(x["specimens"] > 0 for x in known)
        assert novel and novel[0]["barcode"] == missing
        second = novel[1]["exact"] if len(novel) > 1 else 0
        assert novel[0]["exact"] >= 10 * second and novel[0]["exact"] >= 100
        assert novel[0]["support"][0] == novel[0]["exact"] and sum(novel[0]["support"]) > novel[0]["exact"]
        assert novel[0]["unmatched_support"] > 0 and novel[0]["nearest"] in listed and not novel[0]["notes"]
        c = prim["counters"]
        assert c["hits"] == c["pruned"] + c["short_read"] + c["short_flank"] + c["ambiguous"] + c["counted"]
        assert f"  {missing}  novel" in out
    tsv = [line.split("\t") for line in open(tmp_path / "s.tsv").read().splitlines()]
    assert tsv[0][:4] == ["primer", "direction", "barcode", "status"]
    assert len(tsv) - 1 == sum(len(p["candidates"]) for p in doc["primers"])
    assert next(row for row in tsv if row[3] == "novel")[2] == f[3]
    # the second sheet lists the withheld forward barcode reverse-complemented
    _run_tool([pf2, sf2, fq, "--json", tmp_path / "rc.json"], capsys)
    from specimux_amd import synth
    fwd = json.load(open(tmp_path / "rc.json"))["primers"][0]
    row = next(x for x in fwd["candidates"] if x["status"] == "novel")
    assert row["barcode"] == f[3] and f"revcomp-of:{synth.revcomp(f[3])}" in row["notes"]


def test_golden_reads(lib, tmp_path, capsys):
    from oracle import specimux_oracle as O
    from specimux_amd.demultiplex import compiled_panel
    P, S = f"{GOLDEN}/primers.fasta", f"{GOLDEN}/specimens.txt"
    both = Both(P, S)
    cp = compiled_panel(both.specimens, both.parameters, both.args, both.prefilter)
    tables = []
    for name in ("sequences.fastq", "sequences_rc.fastq"):
        reads, _ = O.read_sequences(f"{GOLDEN}/{name}")
        windows, lens = windows_of(cp, reads)
        table, counters, hits = device_flank(cp, [(windows, lens, None)], want_hits=True)
        want, want_counters, _r = brute_force(cp, windows, lens, hits)
        assert table == want and np.array_equal(counters, want_counters)
        assert_counter_rules(table, counters)
        tables.append(table)
    assert tables[0] == tables[1] and tables[0]
    Lb = int(cp.desc.barcode_len_max)
    assert any((key >> 52 & 31) < Lb for key in tables[0])       # barcodes truncated at the read start: flen < Lb
    gz = tmp_path / "sequences.fastq.gz"
    with open(f"{GOLDEN}/sequences.fastq", "rb") as src, gzip.open(gz, "wb") as dst:
        shutil.copyfileobj(src, dst)
    outs = []
    for tag, seqfile in (("a", f"{GOLDEN}/sequences.fastq"), ("b", f"{GOLDEN}/sequences.fastq"), ("gz", gz)):
        text = _run_tool([P, S, seqfile, "--min-count", "2", "--report", tmp_path / f"{tag}.tsv", "--json", tmp_path / f"{tag}.json"],
                         capsys)
        outs.append((text, open(tmp_path / f"{tag}.tsv", "rb").read(), open(tmp_path / f"{tag}.json", "rb").read()))
    assert outs[0] == outs[1] == outs[2]
    assert json.loads(outs[0][2])["reads"] == 40
