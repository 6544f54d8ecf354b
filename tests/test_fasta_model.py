"""tests/fasta_model.py against the 2.1.4 binary's own answers (tests/golden/fasta_binary.json, made by tests/make_fasta_golden.py):
exit status, messages and .fai of `lofreq faidx`, the reference column `plpsummary` prints (the fetch, up to case), the .gzi of the
BGZF files, `checkref`, and what a stale .fai fetches.  No GPU, no library."""
import json
import os
import struct
import zlib

import pytest

import fasta_model as fm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "fasta_binary.json")))


def bgzf_tables(comp):
    """block tables of a BGZF file: comp_off, data_off, and the inflated bytes"""
    comp_off, data_off, data, at = [0], [0], b"", 0
    while at < len(comp):
        bsize = struct.unpack_from("<H", comp, at + 16)[0] + 1
        data += zlib.decompress(comp[at + 18:at + bsize - 8], -15)
        at += bsize
        comp_off.append(at)
        data_off.append(len(data))
    return comp_off, data_off, data


def test_fixture_covers_the_rules():
    names = {c["name"] for c in GOLD["cases"]}
    assert len(names) == len(GOLD["cases"]) >= 40
    assert {c["status"] for c in GOLD["cases"]} == {0, 1}
    assert any(len(b["cuts"]) >= 4 for b in GOLD["bgzf"]) and len(GOLD["stale"]) >= 2


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_faidx(case):
    m = fm.build(case["text"].encode("latin-1"))
    assert m["status"] == case["status"]
    assert m["log"] == case["messages"]
    if case["status"] == 0:
        assert m["fai"].decode("latin-1") == case["fai"]
        assert m["n_dup"] == sum("duplicate" in x for x in case["messages"])
    else:
        assert m["why"] in (fm.UNEXPECTED, fm.LINE_LENGTH, fm.LAST_EMPTY, fm.EMPTY_FILE)
        if m["why"] == fm.UNEXPECTED:
            assert (" at line %d" % m["line"]) in case["messages"][0]
        assert (m["why"] == fm.LINE_LENGTH) == any(x.startswith("Different line length") for x in case["messages"])


@pytest.mark.parametrize("case", [c for c in GOLD["cases"] if "columns" in c], ids=lambda c: c["name"])
def test_fetch_is_the_reference_column(case):
    data = case["text"].encode("latin-1")
    for e in fm.build(data)["entries"]:
        if e[0] and e[1]:
            assert fm.fetch(data, e).decode("latin-1").upper() == case["columns"][e[0].decode("latin-1")]


@pytest.mark.parametrize("case", GOLD["bgzf"], ids=lambda c: c["name"])
def test_bgzf(case):
    comp_off, data_off, data = bgzf_tables(bytes.fromhex(case["comp_hex"]))
    assert data == case["text"].encode("latin-1")
    assert fm.build(data)["fai"].decode("latin-1") == case["fai"]
    assert fm.gzi(comp_off, data_off).hex() == case["gzi_hex"]
    cuts = set(case["cuts"])
    if case["name"] == "four_blocks":           # the cuts the fixture promises: in a header, in a line, on a newline
        first_nl = data.index(b"\n")
        assert any(c < first_nl for c in cuts) and any(data[c - 1:c] == b"\n" for c in cuts)
        assert any(data[c - 1:c] != b"\n" and data[c:c + 1] != b"\n" and c > first_nl for c in cuts)


@pytest.mark.parametrize("case", GOLD["checkref"], ids=lambda c: c["name"])
def test_checkref(case):
    entries = fm.build(case["text"].encode("latin-1"))["entries"]
    bad, why = fm.checkref(entries, [s[0] for s in case["sq"]], [s[1] for s in case["sq"]])
    assert (bad < 0) == (case["status"] == 0)
    if bad >= 0:
        assert case["sq"][bad][0] in case["messages"][-1]
        assert (why == fm.LENGTH) == ("length mismatch" in case["messages"][-1])


@pytest.mark.parametrize("case", GOLD["stale"], ids=lambda c: c["name"])
def test_stale_index(case):
    new = case["new"].encode("latin-1")
    entries = fm.parse_fai(case["fai"].encode("latin-1"))
    got = {e[0].decode("latin-1"): fm.fetch(new, e) for e in entries}
    if case["plpsummary_status"] == 0:
        assert {k: v.decode("latin-1").upper() for k, v in got.items()} == case["columns"]
    else:                                       # the binary gives up at the first contig it cannot fetch
        assert got[entries[0][0].decode("latin-1")] is None
