"""lofreq_amd/csrc/lfq_fasta.h on the host: lfq_fasta_check.cpp, the header's stand-alone program, is compiled with the host compiler
-- plainly, and with the address and undefined-behaviour sanitizers -- and run over the table of tests/fasta_edges.py and every text
of tests/golden/fasta_binary.json.  The expected answers are tests/fasta_model.py's, which tests/test_fasta_model.py holds to the
reference's binary.  The program also holds the kernels' chunk masks to a byte loop on every row.  No GPU and no Python-loaded
library."""
import json
import os
import shutil
import subprocess

import pytest

import fasta_edges as fe
import fasta_model as fm
from test_fasta_model import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")


def _compile(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp), name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags
                       + [os.path.join(CSRC, "lfq_fasta_check.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


def all_rows():
    """{"name", "data", "fai"} of everything the program is run over"""
    rows = [{"name": r["name"], "data": r["data"], "fai": r["fai"]} for r in fe.ROWS]
    rows += [{"name": "golden_" + c["name"], "data": c["text"].encode("latin-1"), "fai": None} for c in GOLD["cases"] + GOLD["bgzf"]]
    rows += [{"name": "stale_" + c["name"], "data": c["new"].encode("latin-1"), "fai": c["fai"].encode("latin-1")} for c in GOLD["stale"]]
    rows += [{"name": "fai_refused_%d" % i, "data": b">a\nAC\n", "fai": t}
             for i, t in enumerate([b"a\t2\t3\n", b"a\tx\t3\t2\t3\n", b"a\t2\t-3\t2\t3\n", b"a\t2\t3\t2\t99999999999\n", b"a\n"])]
    return rows


def want_of(row):
    if row["name"].startswith("fai_refused"):
        return {"parse_error": 1}
    m, fetched = fe.expected(row)
    if row["fai"] is None and m["status"] != 0:
        return {"error": [m["why"], m["line"], m["byte"]], "masks": 1}
    entries = [e for e, _, _ in fetched]
    seen, first = set(), []
    for e in entries:                           # the first of equal names wins in a parsed index too
        if e[0] not in seen:
            seen.add(e[0])
            first.append(e)
    fai = b"".join(e[0] + b"\t%d\t%d\t%d\t%d\n" % e[1:] for e in first)
    return {"fai": fai.hex(), "n_dup": (len(entries) - len(first)) if row["fai"] is not None else m["n_dup"],
            "fetch": [None if fm.fetch(row["data"], e) is None else fm.fetch(row["data"], e).hex() for e in first], "masks": 1}


def run_rows(exe, rows):
    text = "".join("%s %s\n" % (r["data"].hex() or "-", "-" if r["fai"] is None else r["fai"].hex()) for r in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = [json.loads(line) for line in p.stdout.split("\n")[:-1]]
    assert len(out) == len(rows)
    return out


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe, r = _compile(tmp_path_factory.mktemp("fasta"), "lfq_fasta_check", [])
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def answers(prog):
    return run_rows(prog, all_rows())


def test_table_is_on_the_edges():
    by = {r["name"]: r for r in fe.ROWS}
    assert (fe.CHUNK, fe.WAVE, fe.TILE) == (16, 1024, 4096) or fe.TILE == fe.THREADS * fe.CHUNK
    for w in (1, 15, 16, 17, 60, 61, 63, 64, 65):
        assert fm.build(by["width_%d" % w]["data"])["entries"][0][3] == w
    assert fm.build(by["width_wider_than_a_tile"]["data"])["entries"][0][3] > fe.TILE
    for r in fe.ROWS:
        d, w = r["data"], r["where"]
        assert d[w["newline"]] == 0x0a if "newline" in w else True
        assert (d[w["header"]] == 0x3e and (w["header"] == 0 or d[w["header"] - 1] == 0x0a)) if "header" in w else True
        assert d[w["cr"]:w["cr"] + 2] == b"\r\n" if "cr" in w else True
        assert len(d) == w["size"] if "size" in w else True
        assert (fm.build(d)["status"] == 1) == bool(w.get("refused"))
    for what, edge in (("chunk", fe.CHUNK), ("wave", fe.WAVE), ("tile", fe.TILE)):
        assert by["newline_ends_%s" % what]["where"]["newline"] == edge - 1
    assert by["header_starts_tile"]["where"]["header"] % fe.TILE == 0
    assert by["crlf_split_across_tile"]["where"]["cr"] % fe.TILE == fe.TILE - 1
    h = by["header_straddles_tiles"]
    assert h["where"]["header"] < fe.TILE < h["data"].index(b"\n", h["where"]["header"])
    assert len(by["scan_two_rounds"]["data"]) > fe.SCAN_LANES * fe.TILE
    assert len(fm.build(by["thousand_one_base"]["data"])["entries"]) == 1000
    # the irregular row and its twin: the same letters, one provably regular, one not
    irr, reg = fe.expected(by["irregular_blanks"])[1][0], fe.expected(by["regular_twin"])[1][0]
    assert irr[1] == reg[1] == by["regular_twin"]["where"]["letters"] and (irr[2], reg[2]) == (False, True)
    assert irr[0][4] == reg[0][4] == 61         # equal line bytes
    # refusals: first, middle and last tile; of two offences the earlier
    for what, why in (("unexpected", fm.UNEXPECTED), ("line_length", fm.LINE_LENGTH), ("cr_alone", fm.UNEXPECTED)):
        tiles = []
        for where in ("first", "middle", "last"):
            r = by["%s_in_%s_tile" % (what, where)]
            m = fm.build(r["data"])
            assert m["why"] == why
            tiles.append(len(b"".join(x + b"\n" for x in r["data"].split(b"\n")[:m["line"] - 1])) // fe.TILE)
        assert tiles[0] == 0 < tiles[1] < tiles[2] == (len(r["data"]) - 1) // fe.TILE
    a, b = fm.build(by["two_offences"]["data"]), fm.build(by["two_offences_other_order"]["data"])
    assert (a["why"], b["why"]) == (fm.LINE_LENGTH, fm.UNEXPECTED)
    got = fe.expected(by["foreign_index_runs_past"])[1]
    assert got[0][1] is not None and got[1][1] is None and got[2][1] is None


def test_every_row_on_the_host(answers):
    for row, got in zip(all_rows(), answers):
        assert got == want_of(row), row["name"]


def test_a_second_run_prints_the_same(prog, answers):
    rows = all_rows()
    assert run_rows(prog, rows[::-1])[::-1] == answers


def test_sanitized_build_runs_clean(tmp_path):
    """the same program under the host compiler's address and undefined-behaviour sanitizers"""
    exe, r = _compile(tmp_path, "lfq_fasta_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link a sanitized program: " + r.stderr[-300:])
    rows = all_rows()
    for row, got in zip(rows, run_rows(exe, rows)):
        assert got == want_of(row), row["name"]
