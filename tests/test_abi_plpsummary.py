"""CPU tests: the ABI of plp_summary's header line -- lfq_readset_plp_summary, lfq_format_plp_summary and
lfq_last_summary_times are declared, bound and exported; NULL arguments are refused without a device; the formatter writes the
reference's line (lofreq_call.c:445-459) from a struct built here, for a base, an insertion and a deletion consensus, and
answers LFQ_ERR_CAPACITY one byte below the room the line needs; ncols = 0 formats nothing; the ABI numbers still agree at 10.
No compute: the device side is tests/test_gpu_plpsummary.py."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFQ_ERR_INVALID, LFQ_ERR_CAPACITY = -1, -4


def test_the_new_symbols_are_declared_bound_and_exported():
    import lofreq_amd as la
    from lofreq_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    assert re.search(r"int lfq_readset_plp_summary\(lfq_ctx \*ctx, lfq_readset \*rs, int64_t region_begin, int64_t region_end, "
                     r"int min_plp_bq,\s*int min_plp_idq, const lfq_plp_summary \*\*out\);", hdr)
    assert "int lfq_format_plp_summary(char *buf, int buflen, const char *chrom, const lfq_plp_summary *summary, int64_t col);" in hdr
    assert "int lfq_last_summary_times(lfq_ctx *ctx, lfq_summary_times *t);" in hdr
    for name in ("lfq_readset_plp_summary", "lfq_format_plp_summary", "lfq_last_summary_times"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    vp = C.c_void_p
    assert L.lfq_readset_plp_summary.argtypes == [vp, vp, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                                  C.POINTER(C.POINTER(_lib.PlpSummaryC))]
    assert L.lfq_last_summary_times.argtypes == [vp, C.POINTER(_lib.SummaryTimes)]
    # the structs as the header lays them out
    assert C.sizeof(_lib.PlpSummaryC) == 15 * 8 and C.sizeof(_lib.SummaryTimes) == 32
    m = re.search(r"typedef struct lfq_plp_summary \{(.*?)\} lfq_plp_summary;", hdr, re.S)
    names = re.findall(r"\*(\w+)", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert ["ncols"] + names == [f[0] for f in _lib.PlpSummaryC._fields_]
    assert callable(la.ReadSet.plp_summary) and callable(la.ReadSet.last_summary_times) and callable(la.format_plp_summary)
    assert "format_plp_summary" in la.__all__


def test_null_arguments_are_refused_before_a_device_is_touched():
    from lofreq_amd import _lib
    L = _lib.load()
    out, st = C.POINTER(_lib.PlpSummaryC)(), _lib.SummaryTimes()
    assert L.lfq_readset_plp_summary(None, None, 0, 10, 3, 0, None) == LFQ_ERR_INVALID
    assert L.lfq_readset_plp_summary(None, None, 0, 10, 3, 0, C.byref(out)) == LFQ_ERR_INVALID
    assert L.lfq_last_summary_times(None, C.byref(st)) == LFQ_ERR_INVALID and L.lfq_last_summary_times(None, None) == LFQ_ERR_INVALID


def _summary(n=3):
    from lofreq_amd.pileup import PlpSummary
    s = PlpSummary.__new__(PlpSummary)
    s.ncols = n
    s.col_pos = np.array([9, 10, 123456788][:n], np.int64)
    s.ref_base = np.frombuffer(b"ANG"[:n], np.uint8).copy()
    s.fw = np.array([[1, 2, 3, 4, 5], [0, 0, 0, 0, 0], [100000, 7, 0, 1, 2]][:n], np.int32).reshape(n, 5)
    s.rv = np.array([[6, 7, 8, 9, 10], [0, 0, 0, 0, 0], [3, 2, 1, 0, 99]][:n], np.int32).reshape(n, 5)
    s.num_heads = np.array([11, 0, 1][:n], np.int32)
    s.num_tails = np.array([12, 0, 2][:n], np.int32)
    s.num_ins = np.array([13, 0, 3][:n], np.int32)
    s.num_dels = np.array([14, 0, 4][:n], np.int32)
    s.hrun = np.array([15, 1, 5][:n], np.int32)
    s.coverage_plp = np.array([55, 1, 100200][:n], np.int32)
    s.cons_kind = np.array([0, 1, 2][:n], np.uint8)
    s.cons_nt = np.frombuffer(b"TAA"[:n], np.uint8).copy()
    s.cons_key_off = np.array([0, 0, 3, 5][:n + 1], np.int64)
    s.cons_key_chars = np.frombuffer(b"ACGTN\0", np.uint8).copy()
    return s


WANT = ["chr7\t10\tA\tT\tA:1/6\tC:2/7\tG:3/8\tT:4/9\tN:5/10\theads:11\ttails:12\tins:13\tdels:14\thrun:15\n",
        "chr7\t11\tN\t+ACG\tA:0/0\tC:0/0\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:1\n",
        "chr7\t123456789\tG\t-TN\tA:100000/3\tC:7/2\tG:0/1\tT:1/0\tN:2/99\theads:1\ttails:2\tins:3\tdels:4\thrun:5\n"]


def test_the_formatter_writes_the_line_of_plp_summary():
    import lofreq_amd as la
    assert la.format_plp_summary("chr7", _summary()) == WANT
    assert la.format_plp_summary(b"chr7", _summary(0)) == []


def test_capacity_at_the_exact_length_and_one_below():
    from lofreq_amd import _lib
    L = _lib.load()
    cs, keep = _summary()._as_c()
    for col, want in enumerate(WANT):
        n = len(want)
        buf = C.create_string_buffer(n + 1)                    # the line and its NUL: fits exactly
        assert L.lfq_format_plp_summary(buf, n + 1, b"chr7", C.byref(cs), col) == n and buf.raw == want.encode() + b"\0"
        small = C.create_string_buffer(n + 1)
        assert L.lfq_format_plp_summary(small, n, b"chr7", C.byref(cs), col) == LFQ_ERR_CAPACITY      # one below
        assert L.lfq_format_plp_summary(small, n - 1, b"chr7", C.byref(cs), col) == LFQ_ERR_CAPACITY
        assert L.lfq_format_plp_summary(small, 0, b"chr7", C.byref(cs), col) == LFQ_ERR_CAPACITY
    buf = C.create_string_buffer(256)
    assert L.lfq_format_plp_summary(buf, 256, b"chr7", C.byref(cs), 3) == LFQ_ERR_INVALID
    assert L.lfq_format_plp_summary(buf, 256, b"chr7", C.byref(cs), -1) == LFQ_ERR_INVALID
    assert L.lfq_format_plp_summary(None, 256, b"chr7", C.byref(cs), 0) == LFQ_ERR_INVALID
    assert L.lfq_format_plp_summary(buf, 256, None, C.byref(cs), 0) == LFQ_ERR_INVALID
    assert L.lfq_format_plp_summary(buf, 256, b"chr7", None, 0) == LFQ_ERR_INVALID
    empty, _ = _summary(0)._as_c()
    assert L.lfq_format_plp_summary(buf, 256, b"chr7", C.byref(empty), 0) == LFQ_ERR_INVALID      # ncols = 0: no column to format


def test_abi_version_is_10_everywhere():
    from lofreq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    assert int(re.search(r"#define LFQ_ABI_VERSION (\d+)", hdr).group(1)) == 10
    assert _lib.LFQ_ABI_VERSION == 10
    assert _lib.load().lfq_abi_version() == 10
    assert "lfq_readset_plp_summary, lfq_format_plp_summary, lfq_last_summary_times are new functions" in hdr
