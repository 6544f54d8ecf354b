"""tests/vcf_model.py against the 2.1.4 binary's own answers (tests/golden/vcf_binary.json, made by tests/make_vcf_golden.py): every
record read and rewritten by `lofreq vcfset -a concat` and by `lofreq filter --no-defaults`, and intersect / complement against a
second file the binary read through the Python-written .tbi.  A row is either byte-equal text plus equal counts, or one of the
refusals lofreq_amd/csrc/lfq_vcf.h adds, listed in REFUSED with what the binary does instead.  No row is skipped.  No GPU, no library."""
import hashlib
import json
import os
import re

import pytest

import vcf_edges as ve
import vcf_model as vm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "vcf_binary.json")))

# the rows the library refuses and the binary does not (or not in the same way): why, and the binary's own behaviour as recorded
REFUSED = {
    "two_offences": (vm.NUMBER, "status 0: atol saturates, the record is written with POS 9223372036854775807"),
    "two_offences_other_order": (vm.NUL, "status 0: the line ends at its NUL for fgets' caller, the rest is lost"),
    "two_offences_on_one_line": (vm.NUL, "status 0: as above"),
    "nul_behind_the_records": (vm.NUL, "status 0: the NUL stands behind the line that ends the records"),
    "pos_zero_in_file_one": (vm.INTERVAL, "status 0: the tabix query c1:0-0 finds nothing, the record counts as not in file 2"),
    "line_of_8191": (vm.LINE_TOO_LONG, "status 0: the line is split, see SPLIT_BY_THE_BINARY"),
    "line_of_8190_and_cr": (vm.LINE_TOO_LONG, "status 0: as above"),
    "multiallelic_behind_the_kind_filter": (vm.MULTIALLELIC, "status != 0: No support for multi-allelic SNVs in vcf1"),
    "multiallelic_in_front_of_only_passed": (vm.MULTIALLELIC, "status != 0: as above"),
    "multiallelic_first_of_two": (vm.MULTIALLELIC, "status != 0: as above"),
    "multiallelic_in_concat_file_two": (vm.MULTIALLELIC, "status != 0: as above"),
}


# The line limit is the LINE_BUF_SIZE 8192 of the vcf.c the rules cite.  The 2.1.4 binary was built with a buffer of half that: it
# splits a line behind 4095 bytes and reads the rest as a line of its own, so these rows differ from it, as recorded
SPLIT_BY_THE_BINARY = {"line_of_8190", "line_of_8191", "line_of_8190_and_cr"}


def same(held, data):
    """is `data` the text the fixture holds (make_vcf_golden.pack: itself, or SHA-1 and length of a long one)?"""
    if isinstance(held, str):
        return held.encode("latin-1") == data
    return (held["sha1"], held["len"]) == (hashlib.sha1(data).hexdigest(), len(data))


def test_fixture_covers_the_rules():
    names = {s["name"] for s in GOLD["sets"]}
    assert "took the Python-written .tbi in" in GOLD["note"] and "rejected it in 0" in GOLD["note"]
    ops = {s["conf"]["op"] for s in GOLD["sets"]}
    assert ops == {vm.INTERSECT, vm.COMPLEMENT, vm.CONCAT}
    for flag in ("only_passed", "only_pos", "only_snvs", "only_indels", "count_only"):
        for op in ("intersect", "complement", "concat"):
            assert "%s_%s" % (op, flag) in names
    assert {"intersect_add_info", "concat_add_info", "multiallelic_behind_the_kind_filter", "multiallelic_in_front_of_only_passed",
            "concat_no_header", "equal_pos_run_of_65"} <= names
    rt = {r["name"]: r for r in GOLD["roundtrip"]}
    assert {"mixed_rules", "mixed_rules_crlf", "short_line_mid_file", "no_chrom_line", "no_final_newline"} <= set(rt)
    one = {r["name"]: r for r in ve.OPEN}["mixed_rules"]["data"].decode("latin-1")
    assert same(rt["mixed_rules"]["text"], one.encode("latin-1"))
    for piece in ("\t007\t", "\t12abc\t", "\t37.9\t", "\t.5\t", "PASSx", "\t.x\t", "q20", "indel=1", "XINDEL", "\tGT\t0/1\n", "c2\t8\t.\tA\tG\n"):
        assert piece in one, piece


@pytest.mark.parametrize("row", GOLD["sets"], ids=lambda s: s["name"])
def test_vcfset_equals_the_binary(row):
    r = {r["name"]: r for r in ve.SETS}[row["name"]]
    assert same(row["one"], r["one"]) and (row["two"] is None) == (r["two"] is None) and (r["two"] is None or same(row["two"], r["two"]))
    assert len(row["more"]) == len(r["more"]) and all(same(a, b) for a, b in zip(row["more"], r["more"]))   # the fixture is this table's
    want = ve.expected_set(r)
    if "why" in want:
        why, _ = REFUSED[row["name"]]
        assert want["why"] == why
        if why == vm.MULTIALLELIC:
            assert row["status"] != 0 and any("multi-allelic" in m for m in row["messages"])
        else:
            assert row["status"] == 0
        return
    assert row["name"] not in REFUSED and "open" not in want
    assert row["status"] == 0, row["messages"]
    n_vars1, n_ignored, n_out = want["counts"]
    if r["conf"]["count_only"]:
        assert same(row["out"], b"%d\n" % n_out)
    else:
        assert same(row["out"], bytes.fromhex(want["text"]))
    parsed = [re.findall(r"\d+", m) for m in row["messages"] if m.startswith("Parsed ")]
    wrote = [re.findall(r"\d+", m) for m in row["messages"] if m.startswith("Wrote ")]
    assert parsed and wrote
    assert [int(parsed[0][0]), int(parsed[0][-1])] == [n_vars1 + n_ignored, n_ignored] and int(wrote[0][-1]) == n_out


@pytest.mark.parametrize("row", GOLD["roundtrip"], ids=lambda s: s["name"])
def test_every_record_read_and_rewritten(row):
    text = {r["name"]: r for r in ve.OPEN}[row["name"]]["data"]
    assert same(row["text"], text)                          # the fixture is this table's
    assert (max(len(x) for _, x in vm.split_lines(text) or [(0, b"")]) > 4095) == (row["name"] in SPLIT_BY_THE_BINARY)
    if row["name"] in SPLIT_BY_THE_BINARY:
        out = row["concat"]["out"]
        assert row["concat"]["status"] == 0 and out["newlines"] == text.count(b"\n") - 1       # ... and its second half ends the records
        assert out["longest"] < 4200
        if row["name"] == "line_of_8190":
            assert len(vm.parse(text).recs) == 3
        return
    try:
        p = vm.parse(text)
    except vm.Refused as e:
        assert REFUSED[row["name"]][0] == e.why and row["concat"]["status"] == 0
        return
    assert row["name"] not in REFUSED
    lines = b"".join(x.written() for x in p.recs)
    assert row["concat"]["status"] == 0 and same(row["concat"]["out"], (p.header if p.hdr_line >= 0 else b"") + lines)
    # `lofreq filter --no-defaults`: the records VCF_VAR_PASSES lets through, a FILTER of at most one byte turned into PASS
    out = b""
    for x in p.recs:
        if x.flags & vm.F_PASSES:
            w = x.written().split(b"\t")
            if len(x.filter) <= 1:
                w[6] = b"PASS"
            out += b"\t".join(w)
    assert row["filter"]["status"] == 0
    if not isinstance(row["filter"]["out"], str):           # a long output, held by its digest: the file's own header in front
        assert p.hdr_line >= 0 and same(row["filter"]["out"], p.header + out)
        return
    got = row["filter"]["out"].encode("latin-1")
    assert got.endswith(out)
    head = got[:len(got) - len(out)]
    assert all(ln.startswith(b"#") for ln in head.split(b"\n") if ln)
    if p.hdr_line >= 0:
        assert head.startswith(p.header[:p.header.rindex(b"#CHROM")])
