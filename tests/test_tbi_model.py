"""tests/tbi_model.py -- the Python restatement of the .tbi rules that every test of lfq_vcf_index_* compares with -- held to the
files the reference's 2.1.4 binary wrote (tests/golden/tbi_binary.json, tests/make_tbi_golden.py): per row the binary's own .vcf.gz,
with its blocks, and its .tbi.  The fixture decides: a rule of the model that disagrees with it is wrong.  Files are compared PARSED:
the binary writes bins in its hash table's order.  No GPU, no library."""
import base64
import json
import os
import re

import pytest

import bai_model as bm
import golden_util as gu
import tbi_edges as te
import tbi_model as tm
import vcf_model as vm


class Fixture:
    def __init__(self, row):
        self.name, self.status, self.messages = row["name"], row["status"], row["messages"]
        self.gz = base64.b64decode(row["gz"])
        self.want = None if row["tbi"] is None else tm.from_json(tm.unpack(row["tbi"]))
        self.text, self.data_off, self.comp_off = bm.file_tables(self.gz)
        try:
            self.got = tm.build(self.text, self.data_off, self.comp_off, 0)
        except vm.Refused as e:
            self.got = (e.why, e.line)


_CACHE = {}


def load():
    """the fixture with the model's index of every row, computed once for every test module that asks"""
    if not _CACHE:
        fx = json.load(open(os.path.join(gu.GOLDEN_DIR, "tbi_binary.json")))
        _CACHE["rows"] = [Fixture(r) for r in fx["rows"]]
        _CACHE["note"] = fx["note"]
    return _CACHE["rows"]


NAMES = [name for name, _ in te.BINARY]


def row(name):
    return [f for f in load() if f.name == name][0]


def test_the_fixture_has_every_row_of_the_table():
    assert [f.name for f in load()] == NAMES
    for f in load():
        assert f.status == 0, f.name                        # (a file the binary cannot index still leaves it with status 0)
        assert max([len(ln) for _, ln in vm.split_lines(f.text)] or [0]) < 4095


@pytest.mark.parametrize("name", NAMES)
def test_model_is_the_binarys_index(name):
    f = row(name)
    if f.want is None:
        assert isinstance(f.got, tuple), name
        assert any("hts_idx" in m for m in f.messages) and any("indexing of o.vcf.gz failed" in m for m in f.messages)
    else:
        assert f.got == f.want, name
        assert f.want["conf"] == tm.CONF and f.want["index"]["n_no_coor"] == 0
        assert tm.parse_tbi(tm.to_bytes(f.got)) == f.want


def test_refusals_are_where_the_binary_wrote_no_index():
    why = {f.name: f.got for f in load() if f.want is None}
    assert why == {"pos_one_above_the_limit": (tm.RANGE, 4), "pos_five_above_the_limit": (tm.RANGE, 3),
                   "end_one_above_the_limit": (tm.RANGE, 3), "file_twice": (vm.UNSORTED, 9)}
    assert "Region 536870912..536870913 cannot be stored in a tbi index" in row("pos_one_above_the_limit").messages[0]
    assert "Region 4..536870913" in row("end_one_above_the_limit").messages[0]
    assert "Chromosome blocks not continuous" in row("file_twice").messages[0]
    assert row("pos_and_end_at_the_limit").want is not None           # POS 2^29 and END=2^29 are taken


def test_the_note_counts_rows_taken_and_refused():
    load()
    n_idx, n_ref = sum(f.want is not None for f in load()), sum(f.want is None for f in load())
    m = re.match(r"of (\d+) rows the binary indexed (\d+), all (\d+) reproduced by tests/tbi_model.py; it wrote no index for (\d+), of "
                 r"which the model refuses (\d+); (\d+) rows differ", _CACHE["note"])
    assert m and [int(x) for x in m.groups()] == [len(NAMES), n_idx, n_idx, n_ref, n_ref, 0]


def test_hash_lines_belong_to_the_chunk_of_the_record_behind_them():
    """the rule of lfq_tbx.h's `offsets`, read off the binary's files"""
    f = row("hash_between_runs")
    p, recs = tm.records(f.text, f.data_off, f.comp_off)
    starts = tm.line_offsets(p, f.data_off, f.comp_off)
    c2 = f.want["index"]["refs"][1]
    assert c2["meta"][0][0] == recs[0][4] and c2["meta"][0][0] < starts[1]     # c2 begins where c1's record ends: at the '#' line
    assert f.want["index"]["refs"][0]["meta"][0][1] == recs[0][4]              # and c1 ends there too: the '#' line is not c1's
    f = row("hash_in_front")
    p, recs = tm.records(f.text, f.data_off, f.comp_off)
    assert f.want["index"]["refs"][0]["meta"][0][0] == tm.line_offsets(p, f.data_off, f.comp_off)[0]   # behind the '#' line in front
    f = row("hash_at_the_end")
    assert f.want["index"]["refs"][0]["meta"][0][1] == bm.voffset(len(f.text), f.data_off, f.comp_off)  # the text's end


def test_header_only_and_empty_files_get_an_index_of_no_names():
    for name in ("header_only", "empty"):
        f = row(name)
        assert f.want == {"names": [], "conf": tm.CONF, "index": {"n_ref": 0, "refs": [], "n_no_coor": 0}} == f.got
        assert f.text.endswith(vm.HEADER + b"\n")           # (`filter` writes a header of its own for an empty input)


@pytest.mark.parametrize("name", [n for n in NAMES])
def test_query_reaches_what_brute_force_finds(name):
    f = row(name)
    if f.want is None:
        return
    p, recs = tm.records(f.text, f.data_off, f.comp_off)
    starts = tm.line_offsets(p, f.data_off, f.comp_off)
    for chrom, beg, end in te.queries(f.text):
        check_cover(f.want, p, recs, starts, chrom, beg, end, tm.query(f.want, chrom, beg, end))


def check_cover(t, p, recs, starts, chrom, beg, end, chunks):
    """the query contract: every record overlapping the region starts inside a chunk, chunks sorted and disjoint, none begins in
    front of the linear value"""
    for i in tm.overlapping(p, recs, chrom, beg, end):
        assert any(c[0] <= starts[i] < c[1] for c in chunks), (chrom, beg, end, i)
    assert all(c[0] < c[1] for c in chunks) and all(a[1] < b[0] for a, b in zip(chunks, chunks[1:])), (chrom, beg, end)
    if chunks:
        lin = t["index"]["refs"][t["names"].index(chrom)]["linear"]
        w = max(beg, 0) >> 14
        assert chunks[0][0] >= (lin[w] if w < len(lin) else 0)
    elif chrom not in t["names"] or end <= beg:
        assert chunks == []
