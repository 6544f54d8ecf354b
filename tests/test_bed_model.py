"""tests/bed_model.py held to the reference's 2.1.4 binary (tests/golden/bed_binary.json, made by tests/make_bed_golden.py): every
BED text of the fixture parses -- or is refused -- as `lofreq plpsummary -l` takes it, the columns the binary prints are the
model's read rule and column rule applied to the columns it prints without -l, and under -d they are BED first, then the cap.
No GPU and no library."""
import json
import os

import numpy as np
import pytest

import bed_model as bm
import golden_util as gu
import maxdepth_model as mm

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bed_binary.json")


def load():
    """-> (fixture, {contig: reads as dicts in file order})"""
    fx = json.load(open(FIXTURE))
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    reads = {name: [] for name, _ in fx["contigs"]}
    for name, pos0, flag, mapq, cg, seq, qual in fx["reads"]:
        reads[name].append({"pos0": pos0, "cigar": gu.parse_cigar(cg), "seq": np.array([code.get(c, 4) for c in seq], np.uint8),
                            "qual": np.array([ord(c) - 33 for c in qual], np.uint8), "mapq": mapq, "reverse": bool(flag & 16)})
    return fx, reads


def unpack(cols):
    """the fixture's packed columns -> {contig: positions}, {contig: base counts} (the latter empty where not stored)"""
    pos = {name: [p for a, b in rng for p in range(a, b)] for name, rng in cols["ranges"].items()}
    return pos, cols.get("nb", {})


def base_counts(reads, keep):
    """{pos0: bases of the kept reads there} (every base of the fixture passes min_plp_bq) and the covered positions"""
    nb, cov = {}, set()
    for r, k in zip(reads, keep):
        if not k:
            continue
        x = r["pos0"]
        for op, l in r["cigar"]:
            if op in "M=X":
                for p in range(x, x + l):
                    nb[p] = nb.get(p, 0) + 1
            if op in "MDN=X":
                cov.update(range(x, x + l))
                x += l
    return nb, cov


def model_columns(reads, iv, max_depth):
    """-> (positions, base counts) of one contig under targets iv (None: no -l) and -d max_depth (None: no cap)"""
    pos = [r["pos0"] for r in reads]
    ends = [bm.endpos(r["pos0"], r["cigar"]) for r in reads]
    cap_ends = [mm.ref_end(r["pos0"], r["cigar"]) for r in reads]
    if iv is None:
        keep = mm.kept(pos, cap_ends, max_depth) if max_depth is not None else np.ones(len(reads), np.uint8)
    else:
        keep = bm.bed_then_cap(iv, pos, ends, max_depth, cap_ends)
    nb, cov = base_counts(reads, keep)
    cols = sorted(p for p in cov if iv is None or bm.overlap(iv, p, p + 1))
    return cols, [nb.get(p, 0) for p in cols]


FX, READS = load()
ROWS = {b["name"]: b for b in FX["beds"]}


def test_the_fixture_has_the_cases():
    assert {"plain", "unsorted", "overlapping_and_duplicate", "both_formats", "track_browser_comment", "tabs_and_blanks", "crlf",
            "empty_line_cut_off", "zero_length", "name_not_in_bam", "contig_without_line", "error_no_number",
            "error_end_below_beg", "error_list_zero", "error_negative"} <= set(ROWS)
    assert sum(len(v) for v in READS.values()) >= 200
    ops = {op for rs in READS.values() for r in rs for op, _ in r["cigar"]}
    assert {"M", "D", "N", "S", "I"} <= ops
    assert any(all(op == "S" for op, _ in r["cigar"]) for r in READS["c1"])


def test_without_a_bed_the_model_pileup_is_the_binary_s():
    pos, nb = unpack(FX["nobed_columns"])
    for name, reads in READS.items():
        cols, cnt = model_columns(reads, None, None)
        assert cols == pos[name] and cnt == nb[name], name
    for run in FX["nobed_capped"]:
        pos, nb = unpack(run["columns"])
        for name, reads in READS.items():
            cols, cnt = model_columns(reads, None, run["max_depth"])
            assert cols == pos.get(name, []) and cnt == nb.get(name, []), (name, run["max_depth"])


@pytest.mark.parametrize("name", [b["name"] for b in FX["beds"] if b["status"] == 0])
def test_columns_are_the_model_applied_to_the_no_bed_columns(name):
    row = ROWS[name]
    bed = bm.parse(row["text"])
    got, _ = unpack(row["columns"])
    all_pos, _ = unpack(FX["nobed_columns"])
    for contig, reads in READS.items():
        iv = bed.get(contig, [])
        # the column rule on the columns the binary prints without -l, restricted to what the kept reads still cover
        keep = bm.keep_reads(iv, [r["pos0"] for r in reads], [bm.endpos(r["pos0"], r["cigar"]) for r in reads])
        _, cov = base_counts(reads, keep)
        want = [p for p, k in zip(all_pos[contig], bm.keep_columns(iv, all_pos[contig])) if k and p in cov]
        assert got.get(contig, []) == want, (name, contig)
        assert want == model_columns(reads, iv, None)[0]


def test_what_the_rows_are_about():
    assert bm.parse(ROWS["unsorted"]["text"]) == bm.parse(ROWS["plain"]["text"])
    assert unpack(ROWS["unsorted"]["columns"]) == unpack(ROWS["plain"]["columns"])
    assert bm.parse(ROWS["empty_line_cut_off"]["text"]) == {"c1": [(100, 160)]}
    assert bm.parse(ROWS["empty_first_line"]["text"]) == {} and unpack(ROWS["empty_first_line"]["columns"])[0] == {}
    assert bm.parse(ROWS["crlf"]["text"]) == {"c1": [(100, 160), (250, 300)], "c2": [(50, 80)]}
    assert bm.parse(ROWS["both_formats"]["text"]) == {"c1": [(100, 160), (205, 206), (260, 261), (330, 331)],
                                                     "c2": [(60, 61), (320, 330)]}
    assert bm.parse(ROWS["track_browser_comment"]["text"]) == {"c1": [(100, 160)], "c2": [(50, 80)]}
    assert bm.parse(ROWS["tabs_and_blanks"]["text"]) == {"c1": [(100, 160), (250, 300)], "c2": [(50, 80)]}
    assert bm.parse(ROWS["overlapping_and_duplicate"]["text"])["c1"] == [(90, 400), (100, 120), (100, 160), (100, 160), (140, 210),
                                                                         (395, 399)]
    # a zero-length interval is no column of its own, and keeps reads that reach across it
    z = unpack(ROWS["zero_length"]["columns"])[0]
    assert 130 not in z["c1"] and "c2" not in z
    assert "c2" not in unpack(ROWS["contig_without_line"]["columns"])[0]


@pytest.mark.parametrize("name", [b["name"] for b in FX["beds"] if b["status"] != 0])
def test_parse_errors_are_refused(name):
    row = ROWS[name]
    assert row["status"] == 1
    with pytest.raises(bm.BedRefused) as e:
        bm.parse(row["text"])
    assert e.value.line == row["text"].count("\n")          # the refused line is the last one of these texts


@pytest.mark.parametrize("name", [b["name"] for b in FX["beds"] if b.get("calls")])
def test_cap_rows_are_bed_then_cap(name):
    row = ROWS[name]
    bed = bm.parse(row["text"])
    for run in row["calls"]:
        pos, nb = unpack(run["columns"])
        for contig, reads in READS.items():
            cols, cnt = model_columns(reads, bed.get(contig, []), run["max_depth"])
            assert cols == pos.get(contig, []) and cnt == nb.get(contig, []), (name, contig, run["max_depth"])


def test_the_order_of_bed_and_cap_shows():
    """six 10M reads, then six 50M reads at c2:300, the target 20 bases in, -d 3: with the BED first the 10M reads are never
    pushed, and the room they would have taken under the cap goes to 50M reads"""
    run = [r for r in ROWS["plain"]["calls"] if r["max_depth"] == 3][0]
    pos, nb = unpack(run["columns"])
    with_bed = dict(zip(pos["c2"], nb["c2"]))
    pos0, nb0 = unpack([r for r in FX["nobed_capped"] if r["max_depth"] == 3][0]["columns"])
    without = dict(zip(pos0["c2"], nb0["c2"]))
    assert with_bed[325] > without[325]
    reads = READS["c2"]
    iv = bm.parse(ROWS["plain"]["text"])["c2"]
    keep = bm.bed_then_cap(iv, [r["pos0"] for r in reads], [bm.endpos(r["pos0"], r["cigar"]) for r in reads], 3,
                           [mm.ref_end(r["pos0"], r["cigar"]) for r in reads])
    plain_cap = mm.kept([r["pos0"] for r in reads], [mm.ref_end(r["pos0"], r["cigar"]) for r in reads], 3)
    at = [i for i, r in enumerate(reads) if r["pos0"] == 300]
    short = [i for i in at if reads[i]["cigar"] == [("M", 10)]]
    long_ = [i for i in at if reads[i]["cigar"] == [("M", 50)]]
    assert len(short) == 6 and len(long_) == 6 and max(short) < min(long_)
    assert not keep[short].any()                                    # off target: never pushed, so they use up none of the cap
    assert keep[long_].sum() > plain_cap[long_].sum()              # ... which the 50M reads get instead
    assert with_bed[325] - without[325] == keep[long_].sum() - plain_cap[long_].sum()
