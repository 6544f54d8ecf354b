"""lofreq_amd/csrc/lfq_bed.h on the host: lfq_bed_check.cpp, the header's stand-alone program, is compiled with the host compiler --
plainly, and with the address and undefined-behaviour sanitizers -- and run over the table of tests/bed_edges.py, the refused and
odd texts there, and the BED texts of tests/golden/bed_binary.json.  The expected answers are tests/bed_model.py's, which
tests/test_bed_model.py holds to the reference's binary.  No GPU and no Python-loaded library."""
import json
import os
import shutil
import subprocess

import pytest

import bed_edges as be
import bed_model as bm
from test_bed_model import FX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")


def _compile(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp), name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags
                       + [os.path.join(CSRC, "lfq_bed_check.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


def all_rows():
    """(name, text, contig, queries) of everything the program is run over"""
    rows = [tuple(r) for r in be.ROWS]
    rows += [("refused_" + n, t, "c1", [(0, 10)]) for n, t, _ in be.REFUSED]
    rows += [("odd_" + n, t, "c1", [(0, 3), (5, 6), (2147483646, 2147483647)]) for n, t, _ in be.ACCEPTED_ODD]
    for b in FX["beds"]:
        for contig, n in FX["contigs"]:
            rows.append(("golden_%s_%s" % (b["name"], contig), b["text"], contig, [(p, p + 1) for p in range(0, n, 7)] + [(0, n)]))
    return rows


def want_of(row):
    _, text, contig, queries = row
    try:
        bed = bm.parse(text)
    except bm.BedRefused as e:
        return {"error": e.line}
    return {"names": [[k, [list(x) for x in v]] for k, v in bed.items()],
            "overlap": [1 if bm.overlap(bed.get(contig, []), b, e) else 0 for b, e in queries]}


def run_rows(exe, rows):
    text = "".join("%s %s %s\n" % (t.encode("latin-1").hex() or "-", contig, ",".join("%d:%d" % q for q in queries) or "-")
                   for _, t, contig, queries in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = [json.loads(line) for line in p.stdout.split("\n")[:-1]]
    assert len(out) == len(rows)
    return out


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe, r = _compile(tmp_path_factory.mktemp("bed"), "lfq_bed_check", [])
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def answers(prog):
    return run_rows(prog, all_rows())


def test_table_has_the_edges():
    names = {r.name for r in be.ROWS}
    for n in (0, 1, 2, 3, 63, 64, 65, 1000):
        row = [r for r in be.ROWS if r.name == "table_of_%d" % n][0]
        assert len(bm.parse(row.text).get("c1", [])) == n
        got = be.expected(row)
        assert n == 0 or (0 in got and 1 in got), n
    assert {"touching_is_no_overlap", "zero_length_at_100", "zero_length_at_101", "zero_length_at_149", "zero_length_at_150",
            "long_early_interval", "in_front_and_behind", "at_int32_max"} <= names
    by = {r.name: be.expected(r) for r in be.ROWS}
    assert by["touching_is_no_overlap"] == [0, 0, 1, 1, 1, 1, 0, 0, 1]
    assert [by["zero_length_at_%d" % x][0] for x in (100, 101, 149, 150)] == [0, 1, 1, 0]     # the read [100, 150)
    assert all(by["zero_length_at_%d" % x][1] == 0 for x in (100, 101, 149, 150))              # never a column
    assert by["long_early_interval"][:6] == [1, 1, 1, 0, 0, 1] and by["long_early_interval_ends_first"][:4] == [1, 1, 1, 0]
    assert by["at_int32_max"][:3] == [1, 0, 1]
    for _, text, line in be.REFUSED:
        with pytest.raises(bm.BedRefused) as e:
            bm.parse(text)
        assert e.value.line == line
    for _, text, want in be.ACCEPTED_ODD:
        assert bm.parse(text) == want


def test_every_row_on_the_host(answers):
    for row, got in zip(all_rows(), answers):
        assert got == want_of(row), row[0]


def test_a_second_run_prints_the_same(prog, answers):
    rows = all_rows()
    assert run_rows(prog, rows[::-1])[::-1] == answers


def test_sanitized_build_runs_clean(tmp_path):
    """the same program under the host compiler's address and undefined-behaviour sanitizers"""
    exe, r = _compile(tmp_path, "lfq_bed_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link a sanitized program: " + r.stderr[-300:])
    rows = all_rows()
    for row, got in zip(rows, run_rows(exe, rows)):
        assert got == want_of(row), row[0]
