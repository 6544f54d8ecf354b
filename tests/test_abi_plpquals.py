"""CPU tests: the ABI of plp_summary's quality lines -- lfq_plp_quals_from_tracks, lfq_format_plp_quals,
lfq_set_indel_arrays_all_columns, lfq_format_plp_indel_quals and lfq_last_plp_quals_times are declared, bound and exported; NULL
arguments are refused without a device; the two formatters write the reference's lines (lofreq_call.c:460-598) from structs built
here, for every decoding rule; the length query, the capacity at the exact length and one below, the refusals; the ABI numbers
still agree at 10.  No compute: the device side is tests/test_gpu_plpquals.py."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFQ_ERR_INVALID, LFQ_ERR_CAPACITY = -1, -4
BAQ, SQ = 1, 4


def test_the_new_symbols_are_declared_bound_and_exported():
    import lofreq_amd as la
    from lofreq_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for decl in ("int lfq_plp_quals_from_tracks(lfq_ctx *ctx, const lfq_tracks *tracks, int tracks_on_device, int64_t col_begin, "
                 "int64_t col_end, const lfq_plp_quals **out);",
                 "int lfq_format_plp_quals(char *buf, int64_t buflen, const lfq_plp_quals *q, int64_t col, int flag);",
                 "int lfq_set_indel_arrays_all_columns(lfq_ctx *ctx, int on);",
                 "int lfq_format_plp_indel_quals(char *buf, int64_t buflen, const lfq_indel_columns *cols, int64_t col);",
                 "int lfq_last_plp_quals_times(lfq_ctx *ctx, lfq_plp_quals_times *t);"):
        assert decl in flat, decl
    for name in ("lfq_plp_quals_from_tracks", "lfq_format_plp_quals", "lfq_set_indel_arrays_all_columns",
                 "lfq_format_plp_indel_quals", "lfq_last_plp_quals_times"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    vp = C.c_void_p
    assert L.lfq_plp_quals_from_tracks.argtypes == [vp, C.POINTER(_lib.Tracks), C.c_int, C.c_int64, C.c_int64,
                                                    C.POINTER(C.POINTER(_lib.PlpQualsC))]
    assert L.lfq_format_plp_quals.argtypes == [C.c_char_p, C.c_int64, C.POINTER(_lib.PlpQualsC), C.c_int64, C.c_int]
    assert L.lfq_format_plp_indel_quals.argtypes == [C.c_char_p, C.c_int64, C.POINTER(_lib.IndelColumnsC), C.c_int64]
    # the structs as the header lays them out
    assert C.sizeof(_lib.PlpQualsC) == 7 * 8 and C.sizeof(_lib.PlpQualsTimes) == 32
    m = re.search(r"typedef struct lfq_plp_quals \{(.*?)\} lfq_plp_quals;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"[\s*,](\w+)(?=[,;])", body) == [f[0] for f in _lib.PlpQualsC._fields_]
    m = re.search(r"typedef struct lfq_plp_quals_times \{(.*?)\} lfq_plp_quals_times;", hdr, re.S)
    assert re.findall(r"[\s*,](\w+)(?=[,;])", m.group(1)) == [f[0] for f in _lib.PlpQualsTimes._fields_]
    for name in ("plp_quals", "format_plp_quals", "format_plp_indel_quals", "last_plp_quals_times", "PlpQuals"):
        assert name in la.__all__ and hasattr(la, name)
    assert callable(la.ReadSet.plpsummary_text) and callable(la.SnvCaller.set_indel_arrays_all_columns)
    assert "The indented quality lines of plp_summary (lofreq_call.c:460-597) are not produced" not in hdr


def test_null_arguments_are_refused_before_a_device_is_touched():
    from lofreq_amd import _lib
    L = _lib.load()
    out, t, st = C.POINTER(_lib.PlpQualsC)(), _lib.Tracks(), _lib.PlpQualsTimes()
    assert L.lfq_plp_quals_from_tracks(None, None, 1, 0, 0, None) == LFQ_ERR_INVALID
    assert L.lfq_plp_quals_from_tracks(None, C.byref(t), 1, 0, 0, C.byref(out)) == LFQ_ERR_INVALID
    assert L.lfq_plp_quals_from_tracks(None, C.byref(t), 0, 0, 0, C.byref(out)) == LFQ_ERR_INVALID
    assert L.lfq_set_indel_arrays_all_columns(None, 1) == LFQ_ERR_INVALID
    assert L.lfq_last_plp_quals_times(None, C.byref(st)) == LFQ_ERR_INVALID and L.lfq_last_plp_quals_times(None, None) == LFQ_ERR_INVALID


def _quals(sq=True, baq=True):
    """columns 5 and 6 of some tracks: A x2, T x1, N x3 | empty | (col 7) C x1"""
    from lofreq_amd.pileup import PlpQuals
    q = PlpQuals()
    q.ncols, q.col_begin = 3, 5
    q.nt_off = np.array([0, 2, 2, 2, 3, 6, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7], np.int64)
    q.bq = np.array([30, 2, 93, 0, 41, 7, 12], np.uint8)
    q.baq = np.array([0, 255, 70, 254, 93, 255, 1], np.uint8) if baq else None
    q.mq = np.array([60, 255, 0, 254, 1, 37, 20], np.uint8)
    q.sq = np.array([254, 255, 0, 253, 254, 13, 255], np.uint8) if sq else None
    return q


NT = {
    (5, BAQ | SQ): "  A\tBQ =\t 30 2\n  A\tBAQ =\t 0 -1\n  A\tMQ =\t 60 255\n  A\tSQ =\t 49314 -1\n"
                   "  T\tBQ =\t 93\n  T\tBAQ =\t 70\n  T\tMQ =\t 0\n  T\tSQ =\t 0\n"
                   "  N\tBQ =\t 0 41 7\n  N\tBAQ =\t 254 93 -1\n  N\tMQ =\t 254 1 37\n  N\tSQ =\t 253 49314 13\n",
    (5, BAQ): "  A\tBQ =\t 30 2\n  A\tBAQ =\t 0 -1\n  A\tMQ =\t 60 255\n  T\tBQ =\t 93\n  T\tBAQ =\t 70\n  T\tMQ =\t 0\n"
              "  N\tBQ =\t 0 41 7\n  N\tBAQ =\t 254 93 -1\n  N\tMQ =\t 254 1 37\n",
    (5, 0): "  A\tBQ =\t 30 2\n  A\tBAQ =\t -1 -1\n  A\tMQ =\t 60 255\n  T\tBQ =\t 93\n  T\tBAQ =\t -1\n  T\tMQ =\t 0\n"
            "  N\tBQ =\t 0 41 7\n  N\tBAQ =\t -1 -1 -1\n  N\tMQ =\t 254 1 37\n",
    (6, BAQ | SQ): "",
    (7, SQ): "  C\tBQ =\t 12\n  C\tBAQ =\t -1\n  C\tMQ =\t 20\n  C\tSQ =\t -1\n",
}


def test_the_nucleotide_lines_of_plp_summary():
    import lofreq_amd as la
    import plpquals_ref as Q
    q = _quals()
    for (col, flag), want in NT.items():
        assert la.format_plp_quals(q, flag, [col]) == [want], (col, flag)
        # ... which is what the restatement prints for these bytes
        assert Q.format_grouped(q.nt_off.tolist(), q.bq, q.baq, q.mq, q.sq, col - q.col_begin, flag) == want
    assert la.format_plp_quals(q, BAQ) == [NT[(5, BAQ)], "", "  C\tBQ =\t 12\n  C\tBAQ =\t 1\n  C\tMQ =\t 20\n"]
    # flags without their array: the reference would read an empty array
    assert la.format_plp_quals(_quals(sq=False), BAQ, [5]) == [NT[(5, BAQ)]]
    assert la.format_plp_quals(_quals(baq=False), 0, [5]) == [NT[(5, 0)]]


def test_nucleotide_lines_length_query_capacity_and_refusals():
    from lofreq_amd import _lib
    L = _lib.load()
    cs, keep = _quals()._as_c()
    for (col, flag), want in NT.items():
        n = len(want)
        assert L.lfq_format_plp_quals(None, 0, C.byref(cs), col, flag) == n            # the length query
        buf = C.create_string_buffer(b"#" * (n + 8), n + 8)
        assert L.lfq_format_plp_quals(buf, n + 1, C.byref(cs), col, flag) == n           # text and NUL fit exactly
        assert buf.raw[:n + 1] == want.encode() + b"\0" and buf.raw[n + 1:] == b"#" * 7
        assert L.lfq_format_plp_quals(buf, n, C.byref(cs), col, flag) == LFQ_ERR_CAPACITY      # one below
        assert L.lfq_format_plp_quals(buf, 0, C.byref(cs), col, flag) == LFQ_ERR_CAPACITY
    buf = C.create_string_buffer(512)
    assert L.lfq_format_plp_quals(buf, 512, None, 5, BAQ) == LFQ_ERR_INVALID
    assert L.lfq_format_plp_quals(buf, 512, C.byref(cs), 4, BAQ) == LFQ_ERR_INVALID      # below col_begin
    assert L.lfq_format_plp_quals(buf, 512, C.byref(cs), 8, BAQ) == LFQ_ERR_INVALID      # past the range
    assert L.lfq_format_plp_quals(buf, 512, C.byref(cs), 0, BAQ) == LFQ_ERR_INVALID      # an index of the range, not of the tracks
    assert L.lfq_format_plp_quals(buf, -1, C.byref(cs), 5, BAQ) == LFQ_ERR_INVALID
    assert L.lfq_format_plp_quals(None, 512, C.byref(cs), 5, BAQ) == LFQ_ERR_INVALID
    no_sq, k1 = _quals(sq=False)._as_c()
    no_baq, k2 = _quals(baq=False)._as_c()
    assert L.lfq_format_plp_quals(buf, 512, C.byref(no_sq), 5, BAQ | SQ) == LFQ_ERR_INVALID
    assert L.lfq_format_plp_quals(buf, 512, C.byref(no_baq), 5, BAQ) == LFQ_ERR_INVALID
    assert L.lfq_format_plp_quals(buf, 512, C.byref(no_baq), 5, SQ) > 0


def _indel_cols():
    """column 0: two insertion events and one deletion event; column 1: no event; column 2: no read passes on either side"""
    from lofreq_amd.indel import IndelColumns
    return IndelColumns.from_columns([
        {"ref": "A", "coverage_plp": 7, "num_non_indels": 3,
         "ins": {"non_fw": 2, "non_rv": 2, "ne_q": [30, 0, -1, 45], "ne_mq": [60, 255, 0, 20],
                 "events": [{"key": "AC", "fw": 1, "rv": 1, "q": [33, 34], "aq": [-1, 50], "mq": [60, 0], "sq": [32767, 12]},
                            {"key": "N", "fw": 1, "rv": 0, "q": [9], "aq": [7], "mq": [255], "sq": [-1]}]},
         "dels": {"non_fw": 3, "non_rv": 3, "ne_q": [1, 2, 3, 4, 5, 6], "ne_mq": [60, 60, 255, 0, 20, 37],
                  "events": [{"key": "GGT", "fw": 0, "rv": 1, "q": [40], "aq": [41], "mq": [42], "sq": [0]}]}},
        {"ref": "C", "coverage_plp": 2, "num_non_indels": 2,
         "ins": {"non_fw": 1, "non_rv": 1, "ne_q": [25, 26], "ne_mq": [60, 30]},
         "dels": {"non_fw": 1, "non_rv": 1, "ne_q": [27, 28], "ne_mq": [60, 30]}},
        {"ref": "G", "coverage_plp": 1, "num_non_indels": 0, "ins": {}, "dels": {}},
    ])


INDEL = [
    "  +0\tIDQ =\t 30 0 -1 45\n  +0\tMQ =\t 60 255 0 20\n"
    "  +AC\tIQ =\t 33 34\n  +AC\tMQ =\t 60 0\n  +AC\tAQ =\t -1 50\n  +AC\tSQ =\t 49314 12\n"
    "  +N\tIQ =\t 9\n  +N\tMQ =\t 255\n  +N\tAQ =\t 7\n  +N\tSQ =\t -1\n"
    "  -0\tIDQ =\t 1 2 3 4 5 6\n  -0\tMQ =\t 60 60 255 0 20 37\n"
    "  -GGT\tIDQ =\t 40\n  -GGT\tMQ =\t 42\n  -GGT\tAQ =\t 41\n  -GGT\tSQ =\t 0\n\n",
    "  +0\tIDQ =\t 25 26\n  +0\tMQ =\t 60 30\n  -0\tIDQ =\t 27 28\n  -0\tMQ =\t 60 30\n\n",
    "  +0\tIDQ =\t\n  +0\tMQ =\t\n  -0\tIDQ =\t\n  -0\tMQ =\t\n\n",
]


def test_the_indel_lines_of_plp_summary():
    import lofreq_amd as la
    import plpquals_ref as Q
    cols = _indel_cols()
    assert la.format_plp_indel_quals(cols) == INDEL
    assert la.format_plp_indel_quals(cols, [1]) == [INDEL[1]]
    # ... which is what the restatement prints for the same values (49314 where rd_sq saturates)
    ne = [[(30, 60), (0, 255), (-1, 0), (45, 20)], [(1, 60), (2, 60), (3, 255), (4, 0), (5, 20), (6, 37)]]
    ev = [{"AC": [(33, 60, -1, 49314), (34, 0, 50, 12)], "N": [(9, 255, 7, -1)]}, {"GGT": [(40, 42, 41, 0)]}]
    assert Q.format_indels(ne, ev) == INDEL[0]
    assert Q.format_indels([[], []], [{}, {}]) == INDEL[2]


def test_indel_lines_length_query_capacity_and_refusals():
    from lofreq_amd import _lib
    L = _lib.load()
    cols = _indel_cols()
    cs = cols.c_struct()
    for col, want in enumerate(INDEL):
        n = len(want)
        assert L.lfq_format_plp_indel_quals(None, 0, C.byref(cs), col) == n
        buf = C.create_string_buffer(b"#" * (n + 8), n + 8)
        assert L.lfq_format_plp_indel_quals(buf, n + 1, C.byref(cs), col) == n
        assert buf.raw[:n + 1] == want.encode() + b"\0" and buf.raw[n + 1:] == b"#" * 7
        assert L.lfq_format_plp_indel_quals(buf, n, C.byref(cs), col) == LFQ_ERR_CAPACITY
        assert L.lfq_format_plp_indel_quals(buf, 0, C.byref(cs), col) == LFQ_ERR_CAPACITY
    buf = C.create_string_buffer(1024)
    assert L.lfq_format_plp_indel_quals(buf, 1024, None, 0) == LFQ_ERR_INVALID
    assert L.lfq_format_plp_indel_quals(buf, 1024, C.byref(cs), 3) == LFQ_ERR_INVALID
    assert L.lfq_format_plp_indel_quals(buf, 1024, C.byref(cs), -1) == LFQ_ERR_INVALID
    assert L.lfq_format_plp_indel_quals(None, 1024, C.byref(cs), 0) == LFQ_ERR_INVALID
    assert L.lfq_format_plp_indel_quals(buf, -1, C.byref(cs), 0) == LFQ_ERR_INVALID
    # device-only arrays (lfq_set_indel_arrays_on_host(ctx, 0)): ne_q / ne_mq are NULL
    dev = cols.c_struct()
    dev.side[0].ne_q = None
    dev.side[0].ne_mq = None
    assert L.lfq_format_plp_indel_quals(buf, 1024, C.byref(dev), 1) == LFQ_ERR_INVALID
    # the all-columns switch off: column 1 has two reads without an event by its counts, and no arrays
    off = _indel_cols()
    for sd in range(2):
        S = off.sides[sd]
        n1 = int(S["ne_off"][2] - S["ne_off"][1])
        S["ne_off"][2:] -= n1
        S["ne_q"], S["ne_mq"] = np.delete(S["ne_q"], range(int(S["ne_off"][1]), int(S["ne_off"][1]) + n1)), \
            np.delete(S["ne_mq"], range(int(S["ne_off"][1]), int(S["ne_off"][1]) + n1))
    cs_off = off.c_struct()
    assert L.lfq_format_plp_indel_quals(buf, 1024, C.byref(cs_off), 1) == LFQ_ERR_INVALID
    assert L.lfq_format_plp_indel_quals(buf, 1024, C.byref(cs_off), 0) == len(INDEL[0])      # an event column has them either way
    assert L.lfq_format_plp_indel_quals(buf, 1024, C.byref(cs_off), 2) == len(INDEL[2])      # nothing to print, nothing missing


def test_abi_version_is_10_everywhere():
    from lofreq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    assert int(re.search(r"#define LFQ_ABI_VERSION (\d+)", hdr).group(1)) == 10
    assert _lib.LFQ_ABI_VERSION == 10
    assert _lib.load().lfq_abi_version() == 10
    assert "lfq_plp_quals_from_tracks, lfq_format_plp_quals, lfq_format_plp_indel_quals, lfq_set_indel_arrays_all_columns, " \
           "lfq_last_plp_quals_times are new functions" in hdr
