"""CPU half of the BAQ boundary tests (tests/baq_edges.py): every table row sits on the boundary it names, and the oracle can
be trusted there -- its HMM equals the reference's kprobaln_ext.c object on every geometry of the table, its tags equal what
the reference's 2.1.4 binary wrote for the table's reads (tests/golden/baq_edges.json)."""
import json
import os

import numpy as np
import pytest

import baq_edges as be
import golden_util as gu

TABLE = be.boundary_table()
FIXTURE = os.path.join(gu.GOLDEN_DIR, "baq_edges.json")


def _row(prefix):
    rows = [r for r in TABLE if r.name.startswith(prefix)]
    assert rows, prefix
    return rows


def test_table_cites_the_sources():
    """every row names a constant that was read from the line it cites, takes the routes it says, and every boundary kind,
    all three routes and both interior states occur"""
    routes, interior = set(), set()
    assert len({be.row_id(r) for r in TABLE}) == len(TABLE)
    for row in TABLE:
        assert row.const in be.C and row.at == be.C[row.const][1], row.name
        exp = be.row_routes(row)
        assert len(exp) == len(row.reads), row.name
        for r, e in zip(row.reads, exp):
            g = be.read_geometry(r, be.REF_LEN)
            assert g.route == e, (row.name, r["name"], g)
            assert g.xb >= 0 and g.xb + g.l_ref <= be.REF_LEN, (row.name, r["name"], g)
        routes |= set(exp)
        for idaq in (False, True):
            ws = be.wavefronts(row.reads, be.REF_LEN, idaq)
            assert sorted(i for _, idx in ws for i in idx) == [i for i, e in enumerate(exp) if e != "wide"]
            states = [be.wave_state(row.reads, idx, rt, be.REF_LEN) for rt, idx in ws]
            interior |= {f_hi > 0 for _, f_hi, _ in states}
            if row.f_hi is not None and not idaq:
                assert states[0][1] == row.f_hi, (row.name, states[0])
    assert {r.kind for r in TABLE} == set(be.KINDS)
    assert routes == {"narrow", "band8", "wide"}
    assert interior == {True, False}
    for c in ("LFQ_BAQ_LDS_MAX_LREF", "LFQ_BAQ_BAND8_CELLS", "LFQ_BAQ_MAX_INDELS", "LFQ_BAQ_MAX_TERMS", "band switch", "xb clamp",
              "xe clamp", "b2", "fh", "f_hi", "batch clamp", "stored rows", "oplen skip", "nflag", "quality table"):
        assert c in {r.const for r in TABLE}, c
    assert (be.LDS_CELLS, be.BAND8_CELLS) == ((2 * 7 + 1) * 3 + 6, (2 * 8 + 1) * 3 + 6)


def test_length_rows():
    """every listed length alone and as a wavefront maximum; Lmax >> 2 and (Lmax >> 2) - 1 reach -1, 0 and 1"""
    single = _row("length: single reads")[0]
    lens = [len(r["seq"]) for r in single.reads]
    assert sorted(lens) == [0] + list(be.LENGTHS) and 0 < lens.index(0) < len(lens) - 1
    lmax = []
    for row in _row("length: wavefront maxima"):
        for route, idx in be.wavefronts(row.reads, be.REF_LEN):
            assert len(idx) == 64 and route == "narrow"
            lmax.append(be.wave_state(row.reads, idx, route, be.REF_LEN)[0])
    assert lmax == list(be.LENGTHS)
    assert {-1, 0, 1} <= {(L >> 2) - 1 for L in lmax} and {0, 1} <= {L >> 2 for L in lmax}
    assert 1 in lmax and any(L % 2 for L in lmax if L > 1) and any(L % 2 == 0 for L in lmax)


def test_interior_rows():
    """the wave minimum of fh on both sides of BWF + 1, set by one lane: by its length, by its clipped window, by its band"""
    f = be.BWF["narrow"]
    got = {}
    for row in _row("interior:"):
        (route, idx), = be.wavefronts(row.reads, be.REF_LEN)
        assert len(idx) == 64
        g = [be.read_geometry(r, be.REF_LEN) for r in row.reads]
        odd = [x for x in g if x.fh != 99]
        assert 1 <= len(odd) <= 2 and len({x.fh for x in odd}) == 1, row.name       # the 100-base reads: fh = 99
        got.setdefault("length" if "bases among" in row.name else "window" if "window cut" in row.name else "band", []).append(odd[0].fh)
        if "window cut" in row.name:
            assert all(len(r["seq"]) > x.l_ref - f and x.b2 == f for r, x in zip(row.reads, g) if x.fh != 99)
        if "bw < 7" in row.name:
            assert odd[0].b2 < f and odd[0].fh == 0
    assert sorted(got["length"]) == [f - 1, f, f + 1, f + 2] and sorted(got["window"]) == [f, f + 1, f + 2] and got["band"] == [0]


def test_short_band_rows():
    """a read of l <= 3 bases whose window a contig end cuts to l + 3 runs with that as its band (4, 5, 6); from 4 bases
    on the cut window holds 7 bases and the band is the default one"""
    ends, wave = _row("bw < 7: reads of 1 to 6")[0], _row("bw < 7: a whole wavefront")[0]
    for r in ends.reads:
        g, l = be.read_geometry(r, be.REF_LEN), len(r["seq"])
        assert g.l_ref == l + 3 and g.b2 == min(l + 3, 7) and g.wr == (2 * g.b2 + 1) * 3 + 6, (r["name"], g)
        assert g.xb == 0 or g.xb + g.l_ref == be.REF_LEN
    assert {be.read_geometry(r, be.REF_LEN).b2 for r in ends.reads} == {4, 5, 6, 7}
    assert all(1 <= be.read_geometry(r, be.REF_LEN).b2 <= 6 for r in wave.reads) and len(wave.reads) == 64


def test_lref_and_width_rows():
    lim = be.MAX_LREF
    alone, mixed = _row("l_ref 300 / 301: alone")[0], _row("l_ref 300 / 301: mixed")[0]
    g = {r["name"]: be.read_geometry(r, be.REF_LEN) for r in alone.reads}
    assert (g["p294"].l_ref, g["p295"].l_ref) == (lim, lim + 1) and g["p294"].wr == g["p295"].wr == be.LDS_CELLS
    assert (g["d1_293"].l_ref, g["d1_294"].l_ref) == (lim, lim + 1)
    assert (g["d2_292"].l_ref, g["d2_293"].l_ref) == (lim, lim + 1) and g["d2_292"].wr == g["d2_293"].wr == be.BAND8_CELLS
    assert g["p295_pos0"].l_ref < lim and g["p295_pos0"].xb == 0
    # in the mixed batch the longest read and the widest row belong to reads the narrow launch does not hold
    gm = [be.read_geometry(r, be.REF_LEN) for r in mixed.reads]
    narrow = [len(r["seq"]) for r, x in zip(mixed.reads, gm) if x.route == "narrow"]
    assert max(len(r["seq"]) for r, x in zip(mixed.reads, gm) if x.route == "wide") >= max(narrow)
    assert max(x.wr for x in gm) > be.LDS_CELLS and narrow.count(150) == 12
    widths = {x.wr for row in _row("wr ") for x in (be.read_geometry(r, be.REF_LEN) for r in row.reads)}
    assert {51, 57, 63} <= widths and max(widths) > 63
    by = {r["name"]: be.read_geometry(r, be.REF_LEN) for r in _row("wr 51 / 57 / 63: deletions and insertions")[0].reads}
    assert by["del8"].bw == 8 + be.BW_ADD and by["del7"].bw == be.BW0 and by["ins8"].bw == 8 + be.BW_ADD
    assert by["ins9_del9"].bw == be.BW0 and by["ins9_del9"].route == "narrow"
    n8 = sum(1 for x in (be.read_geometry(r, be.REF_LEN) for r in _row("wr 51 / 57 / 63: band-7")[0].reads) if x.route == "band8")
    assert 0 < n8 < 64 < len(_row("wr 57:")[0].reads)


def test_clip_rows():
    """both clip rows reach every route; band 8 is reached with l_query - l_ref == 8 and no deletion"""
    for row in _row("clips:"):
        g = [be.read_geometry(r, be.REF_LEN) for r in row.reads]
        assert {x.route for x in g} == {"narrow", "band8", "wide"}
        assert not any(be.has_indel(r) for r in row.reads)
        assert any(x.route == "band8" and len(r["seq"]) - x.l_ref == 8 for r, x in zip(row.reads, g))
        assert all(x.l_ref < len(r["seq"]) for r, x in zip(row.reads, g) if x.route != "narrow")
        assert all(x.xb == 0 or x.xb + x.l_ref == be.REF_LEN for x in g)


def test_idaq_rows():
    """the table restatement: 16 is tracked and 17 is not, the first-operation skips, both clamps of nt, exactly 64 / 65
    indels and exactly 1024 / more than 1024 terms"""
    tab = lambda r: be.idaq_table(r, be.CONTIG, be.REF_LEN)
    e = {r["name"]: r for r in _row("idaq: indels of 16 and 17")[0].reads}
    assert [len(tab(e[n])) for n in ("ins16", "ins17", "del16", "del17", "ins_first", "del_first", "hardclip_then_del")] == [1, 0, 1, 0, 0, 0, 0]
    # (a soft clip advances the query: the deletion behind it has qpos = the clip's length and is tracked)
    assert [x[:2] for x in tab(e["clip_then_del"])] == [("D", 5)]
    assert len(tab(e["ins17_then_del2"])) == 1 and len(tab(e["clip_then_ins"])) == 1 and len(tab(e["ins_last"])) == 1
    (_, qpos, nt, _), = tab(e["ins_run_to_l_query"])
    assert nt == len(e["ins_run_to_l_query"]["seq"]) - qpos and nt > 20             # cut at l_query
    (_, qpos, nt, _), = tab(e["del_run_to_xe"])
    g = be.read_geometry(e["del_run_to_xe"], be.REF_LEN)
    assert nt == len(e["del_run_to_xe"]["seq"]) - qpos + 1 and g.xb + g.l_ref < be.HOMO_AT + be.HOMO_LEN
    (_, qpos, nt, _), = tab(e["del_run_to_contig_end"])
    assert be.read_geometry(e["del_run_to_contig_end"], be.REF_LEN).xb + be.read_geometry(e["del_run_to_contig_end"], be.REF_LEN).l_ref == be.REF_LEN
    assert {op for op, _ in e["eq_x_ops"]["cigar"]} == {"=", "X", "I", "D"} and len(tab(e["eq_x_ops"])) == 2
    r64 = _row("idaq: exactly 64 indels")[0]
    assert [len(tab(r)) for r in r64.reads[:1]] == [be.MAX_INDELS] and all(x[3] for x in tab(r64.reads[0])) and not r64.overflow
    r65 = _row("idaq: 65 indels")[0]
    n = [(len(tab(r)), sum(1 for x in tab(r) if not x[3])) for r in r65.reads if be.has_indel(r)]
    assert n.count((be.MAX_INDELS + 1, 1)) == 64 and n.count((be.MAX_INDELS + 2, 2)) == 1 and r65.overflow
    at, over = _row("idaq: deletions in the homopolymer that need exactly")[0], _row("idaq: deletions in the homopolymer that need a few more")[0]
    for r in at.reads[:2]:
        assert sum(x[2] for x in tab(r)) == be.MAX_TERMS and all(x[3] for x in tab(r)), r["name"]
    assert {be.read_geometry(r, be.REF_LEN).route for r in at.reads[:2]} == {"band8", "wide"}
    for r, extra in zip(over.reads[:4], (1, 2, 7, 40)):
        t = tab(r)
        assert sum(x[2] for x in t) == be.MAX_TERMS + extra and sum(1 for x in t if not x[3]) >= 1, r["name"]
        assert sum(x[2] for x in t if x[3]) <= be.MAX_TERMS and len(t) < be.MAX_INDELS
    assert not at.overflow and over.overflow
    for row in TABLE:                   # no other row runs past a cap
        if not row.overflow:
            assert all(x[3] for r in row.reads for x in tab(r)), row.name
    clean, with_n = _row("idaq: a wavefront of indel reads without")[0], _row("idaq: a wavefront of indel reads over")[0]
    for row, want in ((clean, False), (with_n, True)):
        assert len(row.reads) == 64 and all(be.has_indel(r) for r in row.reads)
        has_n = False
        for r in row.reads:
            g = be.read_geometry(r, be.REF_LEN)
            has_n = has_n or b"N" in be.CONTIG[g.xb:g.xb + g.l_ref].upper() or bool((r["seq"] > 3).any())
        assert has_n == want


def test_quality_row():
    row = _row("quality:")[0]
    seen = {(int(r["qual"][i]), i) for r in row.reads for i in (0, 47, len(r["seq"]) - 1) if len(r["seq"]) == 100}
    for q in (0, 1, 2, 93, 255):
        assert {(q, 0), (q, 47), (q, 99)} <= seen
    assert all(be.read_geometry(r, be.REF_LEN).fh > 47 for r in row.reads if len(r["seq"]) == 100)      # row 48 is interior


def test_contig():
    g = be.CONTIG
    assert g[be.HOMO_AT:be.HOMO_AT + be.HOMO_LEN] == b"A" * be.HOMO_LEN and be.HOMO_LEN >= 300
    assert g[be.AT_AT:be.AT_AT + be.AT_LEN] == b"AT" * (be.AT_LEN // 2)
    assert g.count(b"N") == 1 and g[be.N_AT:be.N_AT + 1] == b"N"
    assert g[be.LOWER_AT:be.LOWER_AT + be.LOWER_LEN].islower() and sum(1 for c in g if chr(c).islower()) == be.LOWER_LEN


def test_oracle_returns_every_read(oracle):
    """no case is left out: the oracle gives lb bytes for every base of every table read, in both modes"""
    for row in TABLE:
        for r in row.reads:
            for extended in (True, False):
                lb, ai, ad = oracle.baq_idaq_read(r["pos0"], r["cigar"], r["seq"], r["qual"], be.CONTIG, extended)
                assert len(lb) == len(r["seq"]), (row.name, r["name"])
                if len(lb):
                    assert 33 <= lb.min() and lb.max() <= 126


def test_hmm_equals_reference_object_on_every_geometry(oracle):
    """every distinct (window, query, qualities, band) of the table through the restated HMM and through the reference's
    kprobaln_ext.c object: probability, states and qualities equal"""
    R = oracle.ref_parts()
    if R is None or not hasattr(R, "kpa_ext_glocal"):
        pytest.skip("oracle/_ref not built (reference tree absent)")
    code = np.full(256, 4, np.uint8)
    for i, c in enumerate("ACGT"):
        code[ord(c)] = code[ord(c.lower())] = i
    seen, bands = set(), set()
    for row in TABLE:
        for r in row.reads:
            if len(r["seq"]) == 0:
                continue
            g = be.read_geometry(r, be.REF_LEN)
            win = code[np.frombuffer(be.CONTIG[g.xb:g.xb + g.l_ref], np.uint8)]
            key = (win.tobytes(), r["seq"].tobytes(), r["qual"].tobytes(), g.bw)
            if key in seen:
                continue
            seen.add(key)
            bands.add(g.b2)
            a = oracle.kpa_glocal(win, r["seq"], r["qual"], bw=g.bw, use_reference=False)
            b = oracle.kpa_glocal(win, r["seq"], r["qual"], bw=g.bw, use_reference=True)
            assert a[0] == b[0], (row.name, r["name"])
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (row.name, r["name"])
    assert len(seen) > 1500 and {4, 5, 6, 7, 8, 9} <= bands


def test_fixture_holds_the_table():
    """tests/golden/baq_edges.json (the 2.1.4 binary's tags; the oracle-vs-binary and GPU-vs-binary tests of test_baq.py and
    test_gpu_baq.py pick it up) holds the table's reads as they are now, and the binary tagged every one it was given"""
    fx, reads = gu.load_baq(FIXTURE)
    assert fx["genome"].encode() == be.CONTIG and fx["alnqual_args"] == []
    table = {(row.name, r["name"]): (row, r) for row in TABLE for r in row.reads}
    assert len(table) == sum(len(row.reads) for row in TABLE)
    raw, beyond = json.load(open(FIXTURE))["reads"], json.load(open(FIXTURE))["reads_beyond_caps"]
    tab = lambda k: be.idaq_table(table[k][1], be.CONTIG, be.REF_LEN)
    assert all(all(x[3] for x in tab((rr["row"], rr["name"]))) for rr in raw)
    assert len(beyond) >= 4 and all(any(not x[3] for x in tab((rr["row"], rr["name"]))) for rr in beyond)
    for rr, r in zip(raw, reads):
        row, t = table[rr["row"], rr["name"]]
        assert (r["pos0"], r["cigar"]) == (t["pos0"], t["cigar"]), rr["name"]
        assert np.array_equal(r["seq"], t["seq"]) and np.array_equal(r["qual"], t["qual"]), rr["name"]
    # only what SAM text cannot hold is missing, and the binary left no read of the length, band, clip and l_ref rows untouched
    cannot = sorted((row.name, r["name"]) for row in TABLE for r in row.reads if len(r["seq"]) == 0 or r["qual"].max() > 93)
    assert sorted(fx["not_in_sam"]) == sorted(n for _, n in cannot) and len(cannot) == 5
    assert fx["untagged"] == []
    if fx["coverage"] == "the whole table":
        assert sorted((rr["row"], rr["name"]) for rr in raw) == sorted(set(table) - set(cannot))
    else:               # the representatives of every row, less what SAM text cannot hold
        want = [(row.name, r["name"]) for row in TABLE for r in be.representatives(row, fx["per_row"])]
        over = {(rr["row"], rr["name"]) for rr in beyond}
        assert [(rr["row"], rr["name"]) for rr in raw] == [k for k in want if k not in cannot and k not in over]
        assert over <= set(want)
        got = {row.name: {be.read_geometry(table[rr["row"], rr["name"]][1], be.REF_LEN).route for rr in raw + beyond if rr["row"] == row.name}
               for row in TABLE}
        for row in TABLE:       # every route a row takes is among its representatives
            assert got[row.name] == set(be.row_routes(row)), row.name
    assert sum(1 for rr in raw if rr["ai"]) >= 30 and sum(1 for rr in raw if rr["ad"]) >= 30


def test_oracle_equals_the_binary_beyond_the_table_caps(oracle):
    """the reads with more indels or repeat cells than the device's table holds: the oracle has no cap and gives the
    binary's lb / ai / ad (the device keeps '~' at the indels its table drops: tests/test_gpu_baq_edges.py)"""
    fx = json.load(open(FIXTURE))
    for rr in fx["reads_beyond_caps"]:
        seq = np.array([be.LETTERS.index(c) for c in rr["seq"]], np.uint8)
        qual = np.array([ord(c) - 33 for c in rr["qual"]], np.uint8)
        lb, ai, ad = oracle.baq_idaq_read(rr["pos0"], gu.parse_cigar(rr["cigar"]), seq, qual, be.CONTIG, True)
        assert lb.tobytes() == rr["lb"].encode(), rr["name"]
        assert (ai is None) == (rr["ai"] is None) and (ad is None) == (rr["ad"] is None), rr["name"]
        assert ai is None or ai.tobytes() == rr["ai"].encode(), rr["name"]
        assert ad is None or ad.tobytes() == rr["ad"].encode(), rr["name"]
