"""The deflate decoder of lfq_bgzf_inflate (lofreq_amd/csrc/lfq_inflate.h) on the host: lfq_inflate_check.cpp, the header's
stand-alone program, is compiled with the host compiler and run over the table of tests/bgzf_edges.py.  The table itself is held to
zlib: a well-formed row inflates to its payload there, a malformed one raises.  No GPU and no Python-loaded library."""
import os
import shutil
import subprocess
import zlib

import pytest

import bgzf_edges as be

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")
STATUS = {"ok": 0, "malformed": 1, "truncated": 2, "overrun": 3, "distance": 4, "size": 5, "crc": 6}


def _compile(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp), name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags
                       + [os.path.join(CSRC, "lfq_inflate_check.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe, r = _compile(tmp_path_factory.mktemp("inflate"), "lfq_inflate_check", [])
    assert r.returncode == 0, r.stderr
    return exe


def _isize(row):
    return row.isize if row.isize is not None else len(row.payload or b"")


def _run(exe, rows):
    """-> per row (status, bytes written, crc, output)"""
    text = "".join("%d %s\n" % (_isize(r), r.raw.hex() or "-") for r in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = p.stdout.split("\n")[:-1]
    assert len(out) == len(rows)
    res = []
    for o in out:
        st, n, crc, hx = o.split()
        res.append((int(st), int(n), int(crc, 16), b"" if hx == "-" else bytes.fromhex(hx)))
    return res


def _check(exe):
    for row, (st, n, crc, data) in zip(be.ROWS, _run(exe, be.ROWS)):
        assert n == len(data) <= _isize(row), row.name
        assert crc == zlib.crc32(data), row.name                # the sliced CRC, whatever the verdict
        if row.verdict == "ok":
            assert st == 0 and data == row.payload, (row.name, st, n)
        elif row.verdict == "deflate":
            assert st in (STATUS["malformed"], STATUS["truncated"], STATUS["distance"]), (row.name, st)
        else:                                                   # the decoder sees isize, the CRC is the caller's compare
            want = row.payload[:_isize(row)]
            assert data == want[:n], row.name
            if row.isize is None:
                assert st == 0 and crc != row.crc, row.name
            elif row.isize < len(row.payload):
                assert st == STATUS["overrun"], (row.name, st)
            else:
                assert st == STATUS["size"] and data == row.payload, (row.name, st)


def test_table_is_held_to_zlib():
    kinds = {"ok": 0, "deflate": 0, "trailer": 0}
    for row in be.ROWS:
        kinds[row.verdict] += 1
        if row.verdict == "deflate":
            assert row.payload is None
            with pytest.raises(zlib.error):
                zlib.decompress(row.raw, -15)
        else:
            assert zlib.decompress(row.raw, -15) == row.payload, row.name
            if row.frameable:
                assert len(be.frame(row)) <= 65536
    assert min(kinds.values()) >= 5, kinds


def test_framing_helper_writes_gzip_members():
    """a framed row is a gzip member to zlib; the end-of-file marker is the specification's 28 bytes"""
    assert be.EOF_BLOCK.hex() == "1f8b08040000000000ff0600424302001b0003000000000000000000"
    for row in be.ROWS:
        if row.verdict == "ok" and row.frameable:
            assert zlib.decompress(be.frame(row), 31) == row.payload, row.name
    assert zlib.decompress(be.EXTRA_SUBFIELD_BLOCK, 31) == be.EXTRA_SUBFIELD_PAYLOAD


def test_hand_built_rows_are_what_they_say():
    by = {r.name: r for r in be.ROWS}
    assert len(by["stored_65535"].raw) == 5 + 65535 and not by["stored_65535"].frameable
    assert b"\x00\x00\xff\xff" in by["stored_empty_from_sync_flush"].raw
    assert by["fixed"].raw[0] & 6 == 2 and by["dynamic_level6"].raw[0] & 6 == 4 and by["stored_level0"].raw[0] & 6 == 0
    for n in (0, 1, 65280, 65536):
        assert len(by["size_%d" % n].payload) == n
    assert len(by["distance_32768"].payload) == 32768 + 10


def test_every_row_on_the_host(prog):
    _check(prog)


def test_sanitized_build_runs_clean(tmp_path):
    """the same program under the host compiler's address and undefined-behaviour sanitizers, malformed rows included"""
    exe, r = _compile(tmp_path, "lfq_inflate_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link a sanitized program: " + r.stderr[-300:])
    _check(exe)
