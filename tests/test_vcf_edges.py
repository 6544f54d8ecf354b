"""lofreq_amd/csrc/lfq_vcf.h on the host: lfq_vcf_check.cpp, the header's stand-alone program, is compiled with the host compiler --
plainly, and with the address and undefined-behaviour sanitizers -- and run over the tables of tests/vcf_edges.py.  The expected
answers are tests/vcf_model.py's.  No GPU and no Python-loaded library."""
import json
import os
import shutil
import subprocess

import pytest

import vcf_edges as ve
import vcf_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")


def _compile(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp), name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags
                       + [os.path.join(CSRC, "lfq_vcf_check.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


def _hex(b):
    return b.hex() if b else "-"


def all_rows():
    """[(name, the program's input line, the model's answer)]"""
    rows = []
    for r in ve.OPEN:
        rows.append((r["name"], "open %d %s" % (r["mode"], _hex(r["data"])), ve.expected_open(r)))
    for r in ve.SETS:
        c = r["conf"]
        line = "set %d %d %d %d %d %d %s %s %s" % (c["op"], c["only_passed"], c["only_pos"], c["only_snvs"], c["only_indels"], c["count_only"],
                                                   _hex(c["add"]), _hex(r["one"]), _hex(r["two"]))
        rows.append((r["name"], " ".join([line] + [_hex(m) for m in r["more"]]), ve.expected_set(r)))
    for r in ve.MASKS:
        bed = "-" if r["bed"] is None else (",".join("%d:%d" % iv for iv in r["bed"]) or "0:0")
        rows.append((r["name"], "mask %s %s %d %s" % (_hex(r["data"]), _hex(r["chrom"]), r["ref_len"], bed),
                     {"mask": vm.ign_mask(vm.parse(r["data"]), r["chrom"], r["ref_len"], r["bed"])}))
    return rows


def run_rows(exe, rows):
    p = subprocess.run([exe], input="".join(line + "\n" for _, line, _ in rows), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = [json.loads(line) for line in p.stdout.split("\n")[:-1]]
    assert len(out) == len(rows)
    return out


@pytest.fixture(scope="module")
def rows():
    return all_rows()


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe, r = _compile(tmp_path_factory.mktemp("vcf"), "lfq_vcf_check", [])
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def answers(prog, rows):
    return run_rows(prog, rows)


def test_table_is_on_the_edges():
    assert (ve.CHUNK, ve.WAVE, ve.TILE, ve.SCAN_LANES) == (16, 1024, 4096, 64) and ve.TILE == ve.THREADS * ve.CHUNK
    by = {r["name"]: r for r in ve.OPEN}
    for what, edge in (("chunk", 13 * ve.CHUNK), ("wave", ve.WAVE), ("tile", ve.TILE)):
        assert edge % ve.CHUNK == 0
        r = by["newline_ends_%s_chrom_line_starts_it" % what]
        assert r["data"][edge - 1] == 0x0a and r["data"][edge:edge + len(vm.HEADER)] == vm.HEADER
        r = by["chrom_line_straddles_%s" % what]
        assert r["data"][edge - 20:edge - 20 + len(vm.HEADER)] == vm.HEADER and r["data"][edge - 21] == 0x0a
        assert vm.parse(r["data"]).hdr_line >= 1
        assert by["tab_ends_%s" % what]["data"][edge - 1] == 0x09 and by["tab_ends_%s" % what]["data"][edge - 4] == 0x0a
        assert by["tab_starts_%s" % what]["data"][edge] == 0x09 and by["tab_starts_%s" % what]["data"][edge - 3] == 0x0a
        r = by["record_ends_%s_without_newline" % what]
        assert len(r["data"]) == edge and r["data"][-1] != 0x0a
    r = by["crlf_split_across_tile"]
    assert r["data"][ve.TILE - 1:ve.TILE + 1] == b"\r\n"
    assert max(len(x) for _, x in vm.split_lines(by["line_of_8190"]["data"])) == 8190
    assert max(len(x) for _, x in vm.split_lines(by["line_of_8191"]["data"])) == 8191
    assert len(by["scan_two_rounds"]["data"]) > ve.SCAN_LANES * ve.TILE and len(by["scan_two_rounds"]["data"]) > 270000
    assert ve.LIST_ROUND == 8192
    for r in ve.OPEN:
        e = ve.expected_open(r)
        assert e.get("why") == r["where"].get("refused"), r["name"]
        if "records" in r["where"]:
            assert e["n_rec"] == r["where"]["records"] > ve.LIST_ROUND and len(e["runs"]) == 3
        if "behind" in r["where"]:
            assert e["behind"] == r["where"]["behind"]
        if "header_line" in r["where"]:
            assert vm.parse(r["data"]).hdr_line == r["where"]["header_line"]
    # refusals: first, middle and last tile; of two offences the earlier
    for what, (mode, why, line) in ve.OFFENCES.items():
        tiles = []
        for where in ("first", "middle", "last"):
            r = by["%s_in_%s_tile" % (what, where)]
            e = ve.expected_open(r)
            start = vm.split_lines(r["data"])[e["line"] - 1][0]
            assert e["why"] == why and start // ve.TILE == r["where"]["first_tile"]
            tiles.append((start // ve.TILE, r["where"]["last_tile"], (len(r["data"]) - 1) // ve.TILE))
        assert tiles[0][0] == 0 < tiles[1][0] < tiles[2][1] == tiles[2][2]
    # vcfset: equal-POS runs, the places of a record of file 1, a CHROM file 2 lacks
    sets = {r["name"]: r for r in ve.SETS}
    for n in (1, 2, 65):
        r = sets["equal_pos_run_of_%d" % n]
        assert sum(1 for x in vm.parse(r["two"], vm.TABIX).recs if (x.chrom, x.pos) == (b"c1", 49)) == n
        assert ve.expected_set(r)["keep"] == r["where"]["keep"]
    assert len(vm.parse(sets["more_records_than_a_scan_round"]["one"]).recs) > 128
    for r in ve.SETS:
        e, w = ve.expected_set(r), r["where"]
        assert "open" not in e, r["name"]
        assert (e.get("why"), e.get("file", 0)) == (w.get("refused"), w.get("file", 0)), r["name"]
        assert "line" not in w or e["line"] == w["line"], r["name"]
    # output lines whose start, POS digits and added string straddle a 16-byte chunk of the output: every phase occurs
    r = sets["output_phases"]
    text = bytes.fromhex(ve.expected_set(r)["text"])
    starts, pos_cut, add_cut = set(), 0, 0
    at = len(vm.parse(r["one"]).header)
    for ln in text[at:].split(b"\n")[:-1]:
        starts.add(at % ve.CHUNK)
        f = ln.split(b"\t")
        p0 = at + len(f[0]) + 1
        pos_cut += p0 // ve.CHUNK != (p0 + len(f[1]) - 1) // ve.CHUNK
        a0 = at + ln.index(r["conf"]["add"])
        add_cut += a0 // ve.CHUNK != (a0 + len(r["conf"]["add"]) - 1) // ve.CHUNK
        at += len(ln) + 1
    assert starts == set(range(ve.CHUNK)) and pos_cut > 10 and add_cut > 10
    masks = {r["name"]: r for r in ve.MASKS}
    assert vm.ign_mask(vm.parse(masks["mask_plain"]["data"]), b"c1", 100) == [0, 1, 49, 59, 98, 99]


def test_every_row_on_the_host(rows, answers):
    for (name, _, want), got in zip(rows, answers):
        assert got == json.loads(json.dumps(want)), name


def test_sanitized_build_runs_clean(tmp_path, rows):
    """the same program under the host compiler's address and undefined-behaviour sanitizers"""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if subprocess.run([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler cannot link a sanitized program at all")
    exe, r = _compile(tmp_path, "lfq_vcf_check_san", san)
    assert r.returncode == 0, r.stderr                      # a compile error that shows only under the sanitizers is a failure
    for (name, _, want), got in zip(rows, run_rows(exe, rows)):
        assert got == json.loads(json.dumps(want)), name
