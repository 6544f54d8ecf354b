"""CPU tests: the host ABI of the VCF index entries -- every symbol resolves and is declared in include/lofreq_amd.h with the signature
the ctypes layer uses, the ABI version is still 10, LFQ_VCF_RANGE is 8 everywhere -- the host-only entries (parse / bytes / names /
query / free) on the .tbi of the reference's 2.1.4 binary (tests/golden/tbi_binary.json) and on the byte strings the parser refuses,
and every LFQ_ERR_INVALID that is promised before a device is touched.  (What lfq_vcf_index_build refuses of an OPEN file needs a
context: tests/test_gpu_vcf_index.py.)"""
import ctypes as C
import os
import re

import pytest

import tbi_edges as te
import tbi_model as tm
from test_tbi_model import NAMES, check_cover, row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFQ_ERR_INVALID = -1
SYMBOLS = {"lfq_vcf_index_build": 8, "lfq_last_vcf_index_times": 2, "lfq_vcf_index_bytes": 3, "lfq_vcf_index_parse": 3,
           "lfq_vcf_index_n_names": 1, "lfq_vcf_index_name": 2, "lfq_vcf_index_query": 7, "lfq_vcf_index_free": 1, "lfq_vcf_open_indexed": 10}


def _lib():
    from lofreq_amd import _lib as m
    return m, m.load()


def content(idx):
    """a VcfIndex in the form tbi_model.build returns"""
    names = idx.names
    return {"names": names, "conf": idx.conf,
            "index": {"n_ref": len(names), "n_no_coor": idx.n_no_coor,
                      "refs": [{"bins": {b: [list(c) for c in cs] for b, cs in idx.bins(n).items()}, "linear": idx.linear(n),
                                "meta": None if idx.meta(n) is None else [list(c) for c in idx.meta(n)]} for n in names]}}


def test_symbols_version_and_declarations():
    m, L = _lib()
    header = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    for s, n_args in SYMBOLS.items():
        assert hasattr(L, s), s
        decl = re.search(r"\b%s\(([^;]*)\);" % s, header)
        assert decl, s
        assert decl.group(1).count(",") + 1 == n_args, s
        assert len(getattr(L, s).argtypes) == n_args, s
    assert L.lfq_abi_version() == 10 and "#define LFQ_ABI_VERSION 10" in header
    assert re.search(r"#define LFQ_VCF_RANGE %d\b" % tm.RANGE, header)
    assert re.search(r"#define LFQ_VC_RANGE %d\b" % tm.RANGE, open(os.path.join(ROOT, "lofreq_amd", "csrc", "lfq_tbx.h")).read())
    assert C.sizeof(m.VcfIndexTimes) == 56


def test_package_exports():
    import lofreq_amd as la
    from lofreq_amd import vcf
    for name in ("VcfIndex", "last_vcf_index_times", "vcf_write_gz"):
        assert hasattr(la, name) and name in la.__all__
    assert vcf.VCF_RANGE == tm.RANGE
    e = la.VcfError(vcf.VCF_RANGE, 0, 12)
    assert (e.why, e.file, e.line) == (tm.RANGE, 0, 12) and "tbi" in str(e)
    for name in ("index", "open_indexed"):
        assert hasattr(la.Vcf, name)


@pytest.mark.parametrize("name", NAMES)
def test_parse_bytes_and_query_of_the_binarys_tbi(name):
    import lofreq_amd as la
    f = row(name)
    if f.want is None:
        return
    idx = la.VcfIndex.from_bytes(tm.to_bytes(f.want))
    assert content(idx) == f.want
    mine = idx.to_bytes()
    assert mine == tm.to_bytes(f.want)
    again = la.VcfIndex.from_bytes(mine)
    assert content(again) == f.want and again.to_bytes() == mine       # bytes -> parse -> bytes
    p, recs = tm.records(f.text, f.data_off, f.comp_off)
    starts = tm.line_offsets(p, f.data_off, f.comp_off)
    for chrom, beg, end in te.queries(f.text):
        got = [list(c) for c in idx.query(chrom, beg, end)]
        assert got == tm.query(f.want, chrom, beg, end), (chrom, beg, end)
        check_cover(f.want, p, recs, starts, chrom, beg, end, got)
    idx.close()
    again.close()


def test_bins_in_hash_order_and_no_trailing_count():
    """any writer's file: the bins of a name the other way round, n_no_coor left off"""
    import lofreq_amd as la
    import struct
    t = tm.parse_tbi(te.GOOD_TBI)
    nm = b"".join(n + b"\0" for n in t["names"])
    out = b"TBI\1" + struct.pack("<8i", len(t["names"]), *t["conf"], len(nm)) + nm
    for r in t["index"]["refs"]:
        out += struct.pack("<i", len(r["bins"]) + 1) + struct.pack("<Ii", 37450, 2) + b"".join(struct.pack("<QQ", *c) for c in r["meta"])
        for b in sorted(r["bins"], reverse=True):
            out += struct.pack("<Ii", b, len(r["bins"][b])) + b"".join(struct.pack("<QQ", *c) for c in r["bins"][b])
        out += struct.pack("<i", len(r["linear"])) + struct.pack("<%dQ" % len(r["linear"]), *r["linear"])
    idx = la.VcfIndex.from_bytes(out)
    assert content(idx) == t and idx.to_bytes() == te.GOOD_TBI
    idx.close()


@pytest.mark.parametrize("name", [n for n, _ in te.PARSE])
def test_parse_refusals(name):
    m, L = _lib()
    data = dict(te.PARSE)[name]
    out = C.c_void_p(7)
    assert L.lfq_vcf_index_parse(data, len(data), C.byref(out)) == LFQ_ERR_INVALID and not out.value


def test_refusals_without_a_device():
    m, L = _lib()
    one = (C.c_int64 * 2)(0, 10)
    out, why, line = C.c_void_p(7), C.c_int(-7), C.c_int64(-7)
    assert L.lfq_vcf_index_build(None, one, one, 1, 0, C.byref(out), C.byref(why), C.byref(line)) == LFQ_ERR_INVALID
    assert not out.value and (why.value, line.value) == (0, 0)          # a refused CALL names no line
    assert L.lfq_vcf_index_build(None, one, one, 1, 0, None, None, None) == LFQ_ERR_INVALID
    assert L.lfq_last_vcf_index_times(None, None) == LFQ_ERR_INVALID
    t = m.VcfIndexTimes()
    assert L.lfq_last_vcf_index_times(None, C.byref(t)) == LFQ_ERR_INVALID
    good = te.GOOD_TBI
    assert L.lfq_vcf_index_parse(None, 0, C.byref(out)) == LFQ_ERR_INVALID
    assert L.lfq_vcf_index_parse(good, -1, C.byref(out)) == LFQ_ERR_INVALID
    assert L.lfq_vcf_index_parse(good, len(good), None) == LFQ_ERR_INVALID
    idx = C.c_void_p()
    assert L.lfq_vcf_index_parse(good, len(good), C.byref(idx)) == 0 and idx.value
    p, n = C.c_void_p(), C.c_int64()
    assert L.lfq_vcf_index_bytes(None, C.byref(p), C.byref(n)) == LFQ_ERR_INVALID
    assert L.lfq_vcf_index_bytes(idx, None, C.byref(n)) == LFQ_ERR_INVALID
    assert L.lfq_vcf_index_bytes(idx, C.byref(p), None) == LFQ_ERR_INVALID
    assert L.lfq_vcf_index_n_names(None) == 0 and L.lfq_vcf_index_n_names(idx) == 2
    assert L.lfq_vcf_index_name(None, 0) is None and L.lfq_vcf_index_name(idx, 2) is None and L.lfq_vcf_index_name(idx, -1) is None
    assert L.lfq_vcf_index_name(idx, 1) == b"c22"
    b, e = C.c_void_p(), C.c_void_p()
    assert L.lfq_vcf_index_query(None, b"c1", 0, 10, C.byref(b), C.byref(e), C.byref(n)) == LFQ_ERR_INVALID
    assert L.lfq_vcf_index_query(idx, None, 0, 10, C.byref(b), C.byref(e), C.byref(n)) == LFQ_ERR_INVALID
    assert L.lfq_vcf_index_query(idx, b"c1", 0, 10, None, C.byref(e), C.byref(n)) == LFQ_ERR_INVALID
    assert L.lfq_vcf_index_query(idx, b"c1", 0, 10, C.byref(b), None, C.byref(n)) == LFQ_ERR_INVALID
    assert L.lfq_vcf_index_query(idx, b"c1", 0, 10, C.byref(b), C.byref(e), None) == LFQ_ERR_INVALID
    assert L.lfq_vcf_index_query(idx, b"absent", 0, 10, C.byref(b), C.byref(e), C.byref(n)) == 0 and n.value == 0
    assert L.lfq_vcf_index_query(idx, b"c1", 9, 9, C.byref(b), C.byref(e), C.byref(n)) == 0 and n.value == 0
    h = C.c_void_p(7)
    comp = b"\0" * 28
    assert L.lfq_vcf_open_indexed(None, comp, len(comp), idx, b"c1", 0, 10, C.byref(h), C.byref(why), C.byref(line)) == LFQ_ERR_INVALID
    assert not h.value and (why.value, line.value) == (0, 0)
    L.lfq_vcf_index_free(idx)
    L.lfq_vcf_index_free(None)
