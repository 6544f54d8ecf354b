"""The host half of lfq_vcf_index_* (lofreq_amd/csrc/lfq_tbx.h): lfq_tbx_check.cpp, the header's stand-alone program, is compiled with
the host compiler -- plainly, and with the address and undefined-behaviour sanitizers -- and run over the table of tests/tbi_edges.py,
over the binary's own files of tests/golden/tbi_binary.json and over the byte strings the parser refuses.  The table itself is held to
tests/tbi_model.py, which tests/test_tbi_model.py holds to the reference's binary.  No GPU and no Python-loaded library."""
import json
import os
import shutil
import subprocess

import pytest

import tbi_edges as te
import tbi_model as tm
from test_tbi_model import check_cover, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")


def _compile(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp), name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags
                       + [os.path.join(CSRC, "lfq_tbx_check.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


def golden_rows():
    """the fixture's files as rows: the binary's text and its real block tables"""
    return [te.Row("golden_" + f.name, f.text, f.data_off, f.comp_off, 0, f.got if isinstance(f.got, tuple) else None) for f in load()]


def all_rows():
    return te.ROWS + golden_rows()


def run_rows(exe, rows, parse=()):
    """-> per row the program's answer: (why, line), or (index in tbi_model.as_json's form, the queries' chunks); per byte string of
    `parse` its answer as printed"""
    csv = lambda xs: ",".join(str(int(x)) for x in xs)
    text = "".join("build %s %s %s %d %s\n" % (r.text.hex() or "-", csv(r.data_off), csv(r.comp_off), r.file_off,
                                               ",".join("%s:%d:%d" % (n.hex(), b, e) for n, b, e in te.queries(r.text)) or "-") for r in rows)
    text += "".join("parse %s\n" % b.hex() for b in parse)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = [json.loads(line) for line in p.stdout.split("\n")[:-1]]
    assert len(out) == len(rows) + len(parse)
    got = [(o["why"], o["line"]) if "why" in o else ({k: o[k] for k in ("names", "conf", "index")}, o["queries"]) for o in out[:len(rows)]]
    return got, out[len(rows):]


def want_of(row):
    e = te.expected(row)
    return e if isinstance(e, tuple) else (tm.as_json(e), [tm.query(e, *q) for q in te.queries(row.text)])


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe, r = _compile(tmp_path_factory.mktemp("tbx"), "lfq_tbx_check", [])
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def answers(prog):
    return run_rows(prog, all_rows(), [b for _, b in te.PARSE] + [te.GOOD_TBI])


def test_table_is_held_to_the_model():
    names = {r.name for r in te.ROWS}
    for n in (1, 63, 64, 65, te.WG - 1, te.WG, te.WG + 1, te.TBX_WG - 1, te.TBX_WG, te.TBX_WG + 1, te.ROUND - 1, te.ROUND, te.ROUND + 1):
        assert "%d_records" % n in names
    assert any(len(te.expected(r)["names"]) > max(te.WG, te.TBX_WG) for r in te.ROWS if r.refused is None)
    assert {"line_starts_a_block", "line_straddles_two_blocks", "file_off_above_zero", "wide_bin_span_65535", "wide_bin_span_65536",
            "hash_in_front", "hash_between_records_of_a_run", "hash_between_runs", "header_only", "empty"} <= names
    for row in te.ROWS:
        got = te.expected(row)
        if row.refused is not None:
            assert got == row.refused, (row.name, got)
        else:
            assert isinstance(got, dict), (row.name, got)
    by = {r.name: te.expected(r) for r in te.ROWS if r.refused is None}
    # rule 6, worked out by hand: at 65 535 compressed bytes bin 4682 goes into its parent 585, at 65 536 it stays
    assert sorted(by["wide_bin_span_65535"]["index"]["refs"][0]["bins"]) == [585]
    assert sorted(by["wide_bin_span_65536"]["index"]["refs"][0]["bins"]) == [585, 4682]
    assert by["file_off_above_zero"]["index"]["refs"][0]["meta"][0][0] >> 16 >= 123456789
    assert by["pos_and_end_at_the_limit"]["index"]["refs"][0]["linear"].__len__() == 1 << 15
    assert {r.refused[0] for r in te.ROWS if r.refused} == {4, 5, 6, 8}


def test_every_row_on_the_host(answers):
    for row, got in zip(all_rows(), answers[0]):
        assert got == want_of(row), row.name


def test_the_binarys_files_on_the_host(answers):
    """the header's passes on the binary's own .vcf.gz: the binary's parsed .tbi"""
    for f, got in zip(load(), answers[0][len(te.ROWS):]):
        if f.want is None:
            assert isinstance(got, tuple) and got == f.got, f.name
        else:
            assert tm.from_json(got[0]) == f.want, f.name


def test_query_contract_on_every_row(answers):
    import vcf_model as vm
    for row, got in zip(all_rows(), answers[0]):
        if isinstance(got, tuple):
            continue
        t = tm.from_json(got[0])
        p, recs = tm.records(row.text, row.data_off, row.comp_off, row.file_off)
        starts = tm.line_offsets(p, row.data_off, row.comp_off, row.file_off)
        for (chrom, beg, end), chunks in zip(te.queries(row.text), got[1]):
            check_cover(t, p, recs, starts, chrom, beg, end, chunks)


def test_parse_refusals_and_the_round_trip(answers):
    for (name, _), got in zip(te.PARSE, answers[1]):
        assert got == {"ok": 0}, name
    good = answers[1][-1]
    assert good["ok"] == 1 and bytes.fromhex(good["bytes"]) == te.GOOD_TBI             # bytes -> parse -> bytes
    assert [bytes.fromhex(n) for n in good["names"]] == [b"c1", b"c22"]


def test_other_writers_settings_are_kept(prog):
    """bins in any order, no trailing n_no_coor, format / columns / meta / skip of another writer: kept and given back"""
    import struct
    odd = te.GOOD_TBI[:8] + struct.pack("<6i", 0, 3, 4, 5, ord("@"), 7) + te.GOOD_TBI[32:-8]
    _, out = run_rows(prog, [], [odd])
    assert out[0]["ok"] == 1 and out[0]["conf"] == [0, 3, 4, 5, ord("@"), 7]
    assert bytes.fromhex(out[0]["bytes"]) == odd + b"\0" * 8


def test_a_second_run_prints_the_same(prog, answers):
    assert run_rows(prog, all_rows()[::-1])[0][::-1] == answers[0]


def test_sanitized_build_runs_clean(tmp_path):
    """the same program under the host compiler's address and undefined-behaviour sanitizers"""
    exe, r = _compile(tmp_path, "lfq_tbx_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link a sanitized program: " + r.stderr[-300:])
    got, parsed = run_rows(exe, all_rows(), [b for _, b in te.PARSE] + [te.GOOD_TBI])
    for row, g in zip(all_rows(), got):
        assert g == want_of(row), row.name
    assert parsed[:-1] == [{"ok": 0}] * len(te.PARSE) and parsed[-1]["ok"] == 1
