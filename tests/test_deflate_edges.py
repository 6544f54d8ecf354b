"""The deflate compressor of lfq_bgzf_deflate (lofreq_amd/csrc/lfq_deflate.h) on the host: lfq_deflate_check.cpp, the header's
stand-alone program, is compiled with the host compiler and run over the table of tests/deflate_edges.py.  The table itself is held
to zlib: level 6 stays within every row's cap, so no cap is one the reference misses.  No GPU and no Python-loaded library."""
import os
import shutil
import subprocess
import zlib

import pytest

import deflate_edges as de

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")


def _compile(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp), name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags
                       + [os.path.join(CSRC, "lfq_deflate_check.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


def run_rows(exe, rows):
    """-> per row (block type, stream, crc of the payload, 1 if the project's inflater gave the payload back)"""
    text = "".join(r.payload.hex() + "\n" for r in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = p.stdout.split("\n")[:-1]
    assert len(out) == len(rows)
    res = []
    for o in out:
        bt, hx, crc, same = o.split()
        res.append((int(bt), bytes.fromhex(hx), int(crc, 16), int(same)))
    return res


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe, r = _compile(tmp_path_factory.mktemp("deflate"), "lfq_deflate_check", [])
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def streams(prog):
    return run_rows(prog, de.ROWS)


def _check(rows, res):
    for row, (bt, stream, crc, same) in zip(rows, res):
        n = len(row.payload)
        assert zlib.decompress(stream, -15) == row.payload, row.name
        assert same == 1, row.name                              # the project's own inflater agrees
        assert crc == zlib.crc32(row.payload), row.name
        assert len(stream) <= 5 + n, (row.name, len(stream))
        if row.cap is not None:
            assert len(stream) <= row.cap, (row.name, len(stream), row.cap)
        assert bt in (0, 1, 2) and stream[0] & 1 == 1 and (stream[0] >> 1) & 3 == bt, (row.name, bt, stream[0])
        if row.btype is not None:
            assert bt == row.btype, row.name
        if bt == 0:
            assert len(stream) == 5 + n and stream[5:] == row.payload, row.name


def test_table_is_held_to_zlib():
    names = {r.name for r in de.ROWS}
    assert {"const", "period300", "sym4", "qual41", "rand256", "distance_32769", "all_256_once", "bam_records"} <= names
    for row in de.ROWS:
        z = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
        s = z.compress(row.payload) + z.flush()
        assert zlib.decompress(s, -15) == row.payload
        if row.cap is not None:
            assert len(s) <= row.cap, (row.name, len(s), row.cap)
    by = {r.name: r for r in de.ROWS}
    assert by["rand256"].btype == 0 and sum(r.cap is not None for r in de.ROWS) == 4
    assert len(by["size_%d" % de.N].payload) == de.N == de.MAX_IN and de.STEP == 64
    assert len(set(by["all_256_once"].payload)) == 256 == len(by["all_256_once"].payload)
    assert by["distance_32769"].payload[:300] == by["distance_32769"].payload[32769:]


def test_every_row_on_the_host(streams):
    _check(de.ROWS, streams)


def test_distance_out_of_reach_is_not_used(streams):
    """32769 random bytes and their first 300 again: 300 more literals keep the stream stored, the match would make it dynamic"""
    by = {r.name: s for r, s in zip(de.ROWS, streams)}
    bt, stream = by["distance_32769"][:2]
    assert bt == 0 and len(stream) == 5 + 32769 + 300


def test_a_second_run_prints_the_same(prog, streams):
    again = run_rows(prog, de.ROWS[::-1])[::-1]                # another order: nothing is left over from the payload before
    assert again == streams


def test_sanitized_build_runs_clean(tmp_path):
    """the same program under the host compiler's address and undefined-behaviour sanitizers"""
    exe, r = _compile(tmp_path, "lfq_deflate_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link a sanitized program: " + r.stderr[-300:])
    _check(de.ROWS, run_rows(exe, de.ROWS))
