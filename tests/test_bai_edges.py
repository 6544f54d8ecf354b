"""The host half of lfq_bam_index_build (lofreq_amd/csrc/lfq_bamidx.h): lfq_bamidx_check.cpp, the header's stand-alone program, is
compiled with the host compiler -- plainly, and with the address and undefined-behaviour sanitizers -- and run over the table of
tests/bai_edges.py and over both BAMs of tests/golden/bai_binary.json.  The table itself is held to tests/bai_model.py, which
tests/test_bai_model.py holds to the reference's binary.  No GPU and no Python-loaded library."""
import json
import os
import shutil
import subprocess

import pytest

import bai_edges as be
import bai_model as bm
from test_bai_model import KINDS, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")


def _compile(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp), name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags
                       + [os.path.join(CSRC, "lfq_bamidx_check.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


def golden_rows():
    """both BAMs of the fixture as rows: the whole inflated file as the body, its real block tables"""
    rows = []
    for kind in KINDS:
        f = load(kind)
        rows.append(be.Row("golden_" + kind, f.data, f.rec_off, f.data_off, f.comp_off, 0, len(f.refs), None, None))
    return rows


def run_rows(exe, rows):
    """-> per row the parsed index as the program prints it (bai_model.as_json's form), or the refused record's number"""
    csv = lambda xs: ",".join(str(int(x)) for x in xs)
    text = "".join("%s %s %s %s %d %d\n" % (bytes(r.body).hex() or "-", csv(r.rec_off), csv(r.data_off), csv(r.comp_off), r.file_off,
                                            r.n_ref) for r in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = [json.loads(line) for line in p.stdout.split("\n")[:-1]]
    assert len(out) == len(rows)
    return [o["error"] if "error" in o else o for o in out]


def want_of(row):
    e = be.expected(row)
    return e if isinstance(e, int) else bm.as_json(e)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe, r = _compile(tmp_path_factory.mktemp("bamidx"), "lfq_bamidx_check", [])
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def answers(prog):
    return run_rows(prog, be.ROWS + golden_rows())


def test_table_is_held_to_the_model():
    names = {r.name for r in be.ROWS}
    assert {"starts_and_ends_on_block_edges", "record_across_three_blocks", "empty_block_between", "last_record_of_the_last_block",
            "ends_on_and_over_every_window_edge", "end_one_above_the_limit", "span_65535_parent_present", "span_65536_parent_present",
            "span_65535_parent_absent", "span_65536_parent_absent", "chunk_starts_in_the_block_the_previous_ends_in",
            "chunk_starts_one_block_behind", "one_run_longer_than_a_workgroup", "only_unmapped_placed_reads_in_a_reference",
            "only_reads_without_coordinates", "one_record", "long_read_then_short_ones_inside_its_span"} <= names
    for n in (63, 64, 65, 129, be.WG + 1):
        assert any(r.name.startswith("%d_records_heads_at_" % n) for r in be.ROWS), n
    assert be.WG % 64 == 0 and any("heads_at_63_64_%d_" % be.WG in r.name for r in be.ROWS)
    refusals = [r for r in be.ROWS if r.error is not None]
    assert len(refusals) >= 16 and {-1, 0, 1, 2, 3, 4, 5} <= {r.error for r in refusals}
    for row in be.ROWS:
        got = be.expected(row)
        if row.error is not None:
            assert got == row.error, (row.name, got)
        else:
            assert isinstance(got, dict), (row.name, got)
            if row.facts:
                row.facts(got)


def test_every_row_on_the_host(answers):
    for row, got in zip(be.ROWS, answers):
        assert got == want_of(row), row.name


@pytest.mark.parametrize("kind", KINDS)
def test_golden_on_the_host(answers, kind):
    """the header's three passes on the fixture's BAMs: the binary's parsed index"""
    got = answers[len(be.ROWS) + KINDS.index(kind)]
    assert bm.from_json(got) == load(kind).want


def test_a_second_run_prints_the_same(prog, answers):
    rows = be.ROWS + golden_rows()
    assert run_rows(prog, rows[::-1])[::-1] == answers


def test_sanitized_build_runs_clean(tmp_path):
    """the same program under the host compiler's address and undefined-behaviour sanitizers"""
    exe, r = _compile(tmp_path, "lfq_bamidx_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link a sanitized program: " + r.stderr[-300:])
    rows = be.ROWS + golden_rows()
    for row, got in zip(rows, run_rows(exe, rows)):
        assert got == (want_of(row) if not row.name.startswith("golden_") else bm.as_json(load(row.name[7:]).want)), row.name
