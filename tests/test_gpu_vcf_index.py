"""GPU tests: the .tbi of a bgzipped VCF built on the device (lfq_vcf_index_build), written and read back (vcf_write_gz, VcfIndex) and a
region opened through it (lfq_vcf_open_indexed), against tests/tbi_model.py on every row of tests/tbi_edges.py and against the files the
reference's 2.1.4 binary wrote (tests/golden/tbi_binary.json): names, bins, chunks, linear index and pseudo-bins; every refusal twice;
the binary's own .vcf.gz inflated and indexed without leaving the device; vcfset through a region open against the whole-file open;
what is launched, and that the compaction shared with lfq_bam_index_build keeps no state between the two."""
import numpy as np
import pytest

import bai_edges as be
import bai_model as bm
import tbi_edges as te
import tbi_model as tm
import vcf_model as vm

from test_abi_vcf_index import content
from test_tbi_model import NAMES, check_cover, row

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
ROWS = {r.name: r for r in te.ROWS}


def _index(la, caller, r):
    v = la.Vcf.open(caller, r.text, tabix=True)
    try:
        return v.index(r.data_off, r.comp_off, r.file_off)
    finally:
        v.close()


@pytest.mark.parametrize("name", [r.name for r in te.ROWS])
def test_every_row_equals_the_model(caller, name):
    import lofreq_amd as la
    r = ROWS[name]
    want = te.expected(r)
    if isinstance(want, tuple):
        assert want == r.refused
        for _ in range(2):                                  # the same first line on two runs
            with pytest.raises(la.VcfError) as e:
                _index(la, caller, r)
            assert (e.value.why, e.value.line) == want, name
        return
    idx = _index(la, caller, r)
    assert content(idx) == want, name
    t = la.last_vcf_index_times(caller)
    n = len(vm.parse(r.text, vm.TABIX).recs)
    assert t["n_records"] == n and t["n_launches"] == (4 if n else 0)
    assert idx.to_bytes() == tm.to_bytes(want)
    for q in te.queries(r.text):
        assert [list(c) for c in idx.query(*q)] == tm.query(want, *q), q
    idx.close()


def test_refused_arguments_of_an_open_file(caller):
    import lofreq_amd as la
    r = ROWS["line_straddles_two_blocks"]
    v = la.Vcf.open(caller, r.text, tabix=True)
    d, c = list(r.data_off), list(r.comp_off)
    bad = [(d[:-1] + [d[-1] + 1], c, 0), (d[:-1] + [d[-1] - 1], c, 0), ([1] + d[1:], c, 0), (d, [c[0], c[1], c[1]], 0), (d, [-1] + c[1:], 0),
           ([d[0], d[2], d[1]][:len(d)], c, 0), (d, c, -1)]
    for dd, cc, fo in bad:
        with pytest.raises(RuntimeError):
            v.index(dd, cc, fo)
        assert la.last_vcf_index_times(caller)["n_launches"] == 0
    assert content(v.index(d, c)) == te.expected(r)
    v.close()
    s = la.Vcf.open(caller, r.text)                         # stream mode: no index
    with pytest.raises(RuntimeError):
        s.index(d, c)
    s.close()


@pytest.mark.parametrize("name", NAMES)
def test_index_of_the_binarys_own_file(caller, name):
    """bgzf_inflate, the text device to device, the index over the inflate result's tables: the binary's .tbi"""
    import lofreq_amd as la
    f = row(name)
    view = la.bgzf_inflate_view(caller, f.gz)
    assert view.data.tobytes() == f.text
    try:
        v = la.Vcf.open(caller, view.data, tabix=True)
    except la.VcfError as e:
        assert f.want is None and (e.why, e.line) == f.got
        return
    assert la.last_vcf_times(caller)["n_from_device"] == 1
    try:
        if f.want is None:
            with pytest.raises(la.VcfError) as e:
                v.index(view.data_off, view.comp_off)
            assert (e.value.why, e.value.line) == f.got == (tm.RANGE, f.got[1])
        else:
            assert content(v.index(view.data_off, view.comp_off)) == f.want      # (the marker's block is in these tables)
    finally:
        v.close()


ONE = te.HEAD + b"".join(te.rec(b"c1", 10 + 7 * i, alt=b"CG"[i % 2:i % 2 + 1]) for i in range(40)) + te.rec(b"c2", 5) + te.rec(b"c9", 5)
TWO = te.HEAD + b"".join(te.rec(b"c1", 10 + 14 * i) for i in range(20)) + te.rec(b"c2", 5, alt=b"T")


def test_write_gz_of_a_vcfset_result(caller):
    import lofreq_amd as la
    one, two = la.Vcf.open(caller, ONE), la.Vcf.open(caller, TWO, tabix=True)
    text = la.vcfset(one, two, op="complement")["text"]
    one.close()
    two.close()
    assert text.count(b"\n") > 20
    gz, tbi_file = la.vcf_write_gz(caller, text)
    data, data_off, comp_off = bm.file_tables(gz)
    assert data == text and gz.endswith(bm.EOF_BLOCK)
    assert la.bgzf_inflate(caller, gz)[0].tobytes() == text
    want = tm.build(text, data_off, comp_off)
    idx = la.VcfIndex.from_file_bytes(caller, tbi_file)
    assert content(idx) == want and tbi_file.endswith(bm.EOF_BLOCK)
    assert bm.file_tables(tbi_file)[0] == tm.to_bytes(want)
    idx.close()
    # blocks end on line boundaries, as the binary's do
    big = te.HEAD + te.run_of(6000)
    gz, tbi_file = la.vcf_write_gz(caller, big)
    data, data_off, comp_off = bm.file_tables(gz)
    assert data == big and len(data_off) > 2 and all(big[o - 1:o] == b"\n" for o in data_off[1:])
    assert content(la.VcfIndex.from_file_bytes(caller, tbi_file)) == tm.build(big, data_off, comp_off)
    assert la.vcf_write_gz(caller, b"")[0] == bm.EOF_BLOCK


def _file_two(la, caller):
    """a second file of two names in many small blocks cut on line boundaries, and its index"""
    lines = [te.rec(b"c1", 100 + 50 * i, info=b"DP=%d" % i) for i in range(1500)] + [te.rec(b"c2", 7 + 1000 * i) for i in range(600)]
    lines[700] = te.rec(b"c1", 100 + 50 * 700, alt=b"G")
    text = te.HEAD + b"".join(lines)
    starts = [s for s, _ in vm.split_lines(text)]
    cuts = starts[2::60]
    comp, comp_off, data_off, _ = la.bgzf_deflate(caller, text, cuts=cuts, eof=True)
    v = la.Vcf.open(caller, text, tabix=True)
    idx = v.index(data_off, comp_off)
    return text, comp.tobytes(), idx, v, len(data_off) - 1


REGIONS = [("first_record_of_a_run", b"c1", 99, 100), ("last_record_of_a_run", b"c1", 100 + 50 * 1499 - 1, 100 + 50 * 1499),
           ("first_record_of_the_second_run", b"c2", 6, 7), ("last_record_of_the_file", b"c2", 7 + 1000 * 599 - 1, 7 + 1000 * 599),
           ("inside_one_block", b"c1", 35000, 35400), ("across_blocks", b"c1", 20000, 45000), ("absent_name", b"c7", 0, 1000),
           ("empty_region", b"c1", 500, 500), ("nothing_there", b"c2", 1 << 28, 1 << 29)]


def test_open_indexed_serves_vcfset_and_the_mask(caller):
    import lofreq_amd as la
    text, comp, idx, whole, n_blocks = _file_two(la, caller)
    assert n_blocks > 20
    p = vm.parse(text, vm.TABIX)
    for name, chrom, beg, end in REGIONS:
        # file 1: the region's own records of file 2 (some with another ALT), and positions file 2 does not have
        inside = [r for r in p.recs if r.chrom == chrom and beg <= r.pos < end][:50]
        one = te.HEAD + b"".join(te.rec(chrom, r.pos + 1, alt=[b"C", b"T"][i % 3 == 2]) + te.rec(chrom, r.pos + 2) for i, r in enumerate(inside))
        if not inside:
            one += te.rec(chrom, max(beg, 0) + 1)
        part = la.Vcf.open_indexed(caller, comp, idx, chrom, beg, end)
        t = la.last_bgzf_times(caller)
        assert part.n_records <= whole.n_records
        if inside:
            assert 0 < t["n_blocks"] < n_blocks, name                 # fewer blocks inflated than the file has
            assert la.last_vcf_times(caller)["n_from_device"] == 1
            assert part.n_records >= len(inside)
        else:
            assert part.n_records == 0 or chrom in (b"c1", b"c2")
        v1 = la.Vcf.open(caller, one)
        for op in ("complement", "intersect"):
            a, b = la.vcfset(v1, part, op=op), la.vcfset(v1, whole, op=op)
            assert a["text"] == b["text"] and a["keep"].tolist() == b["keep"].tolist(), (name, op)
            assert (a["n_out"] > 0) == (op == "complement" or bool(inside)), (name, op)
        v1.close()
        lo, hi = max(beg, 0), min(max(end, 0), 1 << 20)
        assert part.ign_mask(chrom, 1 << 20)[lo:hi].tolist() == whole.ign_mask(chrom, 1 << 20)[lo:hi].tolist(), name
        part.close()
    # another file's index: chunks that do not lie on this file's blocks
    with pytest.raises(RuntimeError):
        la.Vcf.open_indexed(caller, comp[:len(comp) // 2], idx, b"c2", 0, 1 << 29)
    whole.close()
    idx.close()


def test_launches_do_not_grow_with_the_records_and_the_bam_index_is_untouched(caller):
    import lofreq_amd as la
    bam_row = [r for r in be.ROWS if r.name == "one_run_longer_than_a_workgroup"][0]
    build_bam = lambda: la.bam_index_build(caller, bam_row.body, bam_row.rec_off, bam_row.data_off, bam_row.comp_off, bam_row.file_off,
                                           bam_row.n_ref).to_bytes()
    alone = build_bam()
    assert alone == bm.to_bytes(be.expected(bam_row))
    seen = []
    for name in ("65_records", "%d_records" % (2 * te.ROUND + 5)):
        idx = _index(la, caller, ROWS[name])
        t = la.last_vcf_index_times(caller)
        seen.append((t["n_launches"], t["n_records"]))
        assert t["n_chunks"] > 0 and t["n_intervals"] > 0 and t["kernels_ms"] > 0
        assert content(idx) == te.expected(ROWS[name])
        assert build_bam() == alone                         # the shared compaction leaks no state, either way round
        assert la.last_bam_index_times(caller)["n_launches"] == 4
        idx.close()
    assert [s[0] for s in seen] == [4, 4] and seen[0][1] == 65 and seen[1][1] == 2 * te.ROUND + 5
    # a refusal leaves nothing behind either
    with pytest.raises(la.VcfError):
        _index(la, caller, ROWS["range_in_the_middle_workgroup"])
    assert la.last_vcf_index_times(caller)["n_launches"] == 1
    assert build_bam() == alone
    assert content(_index(la, caller, ROWS["65_records"])) == te.expected(ROWS["65_records"])
