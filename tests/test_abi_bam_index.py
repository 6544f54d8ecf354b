"""CPU tests of the host-only entries of the BAM index through the C ABI, with no device: lfq_bam_index_parse / _bytes / _query /
_free on the .bai the reference's 2.1.4 binary wrote (tests/golden/bai_binary.json), lfq_bam_record_chain and lfq_bam_record_cuts
against the loops they replace, and every argument refusal of these entries.  (lfq_bam_index_build needs a context to tell its
own refusals apart: tests/test_gpu_bam_index.py runs them from the table of tests/bai_edges.py.)"""
import ctypes as C
import struct

import numpy as np
import pytest

import bai_edges as be
import bai_model as bm
from test_bai_model import KINDS, check_cover, load

LFQ_ERR_INVALID = -1


def content(idx):
    """a BamIndex in the form bai_model.parse_bai returns"""
    return {"n_ref": idx.n_ref, "n_no_coor": idx.n_no_coor,
            "refs": [{"bins": {b: [list(c) for c in cs] for b, cs in idx.bins(t).items()}, "linear": idx.linear(t),
                      "meta": None if idx.meta(t) is None else [list(c) for c in idx.meta(t)]} for t in range(idx.n_ref)]}


@pytest.mark.parametrize("kind", KINDS)
def test_parse_of_the_binarys_bai(kind):
    import lofreq_amd as la
    f = load(kind)
    idx = la.BamIndex.from_bytes(f.bai)
    assert content(idx) == f.want
    assert idx.meta(1) is None and idx.bins(1) == {} and idx.linear(1) == [] and idx.n_no_coor == 7
    # the library's own file: bins ascending, the pseudo-bin last; parse -> bytes -> parse is the identity
    mine = idx.to_bytes()
    assert mine == bm.to_bytes(f.want) and len(mine) == len(f.bai) and mine != f.bai      # (the binary: its hash table's order)
    again = la.BamIndex.from_bytes(mine)
    assert content(again) == f.want and again.to_bytes() == mine
    idx.close()
    again.close()


@pytest.mark.parametrize("kind", KINDS)
def test_query_covers_the_regions(kind):
    import lofreq_amd as la
    f = load(kind)
    idx = la.BamIndex.from_bytes(f.bai)
    check_cover(f, lambda tid, beg, end: [list(c) for c in idx.query(tid, beg, end)], idx.linear)
    for tid, beg, end in [(0, 0, 1 << 29), (0, 1015808, 1032192), (2, 60000, 190000), (1, 0, 50000), (3, 7, 7), (3, 9, 2), (4, 0, 5000),
                          (0, -5, 10), (0, (1 << 29) - 1, 1 << 40)]:
        assert [list(c) for c in idx.query(tid, beg, end)] == bm.query(f.want, tid, beg, end), (tid, beg, end)
    assert idx.query(1, 0, 50000) == [] and idx.query(3, 7, 7) == []
    idx.close()


def test_record_chain_is_the_fixtures_walk():
    import lofreq_amd as la
    from lofreq_amd import _lib
    L = _lib.load()
    f = load("python")
    first = f.rec_off[0]
    assert la.bam_record_chain(f.data, first).tolist() == f.rec_off
    # a chunk that ends inside a record, inside a block_size, and on a record's end
    for stop in (f.rec_off[10] + 50, f.rec_off[10] + 2, f.rec_off[10]):
        assert la.bam_record_chain(f.data, first, stop).tolist() == f.rec_off[:11] == bm.record_chain(f.data, first, stop)
    assert la.bam_record_chain(f.data, first, first).tolist() == [first]
    p, n = C.POINTER(C.c_int64)(), C.c_int64(5)
    a = np.frombuffer(f.data, np.uint8)
    bad = a[first:first + 200].copy()
    bad[:4] = np.frombuffer(struct.pack("<i", 31), np.uint8)
    for args in ((None, 0, 10), (a.ctypes.data, -1, 10), (a.ctypes.data, 10, 9), (bad.ctypes.data, 0, 200)):
        assert L.lfq_bam_record_chain(args[0], args[1], args[2], C.byref(p), C.byref(n)) == LFQ_ERR_INVALID and not p
    assert L.lfq_bam_record_chain(a.ctypes.data, 0, 10, None, C.byref(n)) == LFQ_ERR_INVALID
    assert L.lfq_bam_record_chain(a.ctypes.data, 0, 10, C.byref(p), None) == LFQ_ERR_INVALID
    L.lfq_bam_record_chain_free(None)


def test_record_cuts_are_the_documented_loop():
    """INTEGRATION.md section 13 prints the loop; tests/bai_model.py's record_cuts is that loop"""
    import lofreq_amd as la
    from lofreq_amd import _lib
    L = _lib.load()
    f = load("python")
    body_off = [o - f.rec_off[0] for o in f.rec_off]
    for piece in (65280, 4096, 119, 120, 1000):
        cuts = la.bam_record_cuts(body_off, piece).tolist()
        assert cuts == bm.record_cuts(body_off, piece), piece
        edges = [0] + cuts + [body_off[-1]]
        assert all(0 < b - a <= piece for a, b in zip(edges, edges[1:]))
        if piece >= 200:                                    # every record fits: every cut is a record boundary, none could be later
            assert set(cuts) <= set(body_off)
            assert all(min(o for o in body_off if o > b) - a > piece for a, b in zip(edges, edges[1:-1]))
    assert la.bam_record_cuts(body_off).tolist() == bm.record_cuts(body_off)
    # a record longer than a piece is cut every max_piece bytes, and the records behind it are kept whole again
    off = [7, 107, 207, 207 + 2500, 2807, 2907]
    assert la.bam_record_cuts(off, 1000).tolist() == [207, 1207, 2207] == bm.record_cuts(off, 1000)
    assert la.bam_record_cuts(off, 250).tolist() == list(range(207, 2458, 250)) + [2707] == bm.record_cuts(off, 250)
    assert la.bam_record_cuts([0, 10], 10).tolist() == [] and la.bam_record_cuts([5], 10).tolist() == []
    assert la.bam_record_cuts([0, 11], 10).tolist() == [10]
    p, n = C.POINTER(C.c_int64)(), C.c_int64()
    ro = np.asarray([0, 10, 10, 30], np.int64)
    for args in ((None, 3, 10), (ro.ctypes.data, -1, 10), (ro.ctypes.data, 3, 0), (ro.ctypes.data, 3, 100)):
        assert L.lfq_bam_record_cuts(args[0], args[1], args[2], C.byref(p), C.byref(n)) == LFQ_ERR_INVALID and not p
    assert L.lfq_bam_record_cuts(ro.ctypes.data, 1, 10, None, C.byref(n)) == LFQ_ERR_INVALID
    L.lfq_bam_record_cuts_free(None)


def test_parse_refuses_what_is_no_bai():
    from lofreq_amd import _lib
    L = _lib.load()
    good = bm.to_bytes(load("python").want)
    one = bm.to_bytes({"n_ref": 1, "n_no_coor": 0, "refs": [{"bins": {4681: [[1, 2]]}, "linear": [1], "meta": [[1, 2], [1, 0]]}]})
    twice = one[:12] + one[12:12 + 24] + one[12:12 + 24] + one[12 + 24:]
    twice = twice[:8] + struct.pack("<i", 3) + twice[12:]
    cases = {"empty": b"", "magic": b"BAM\1" + good[4:], "n_ref_negative": good[:4] + struct.pack("<i", -1) + good[8:],
             "n_ref_past_the_file": good[:4] + struct.pack("<i", 1 << 30) + good[8:], "cut_short": good[:-9],
             "bytes_left_over": good + b"\0", "n_bin_past_the_file": good[:8] + struct.pack("<i", 1 << 28) + good[12:],
             "n_chunk_past_the_file": one[:16] + struct.pack("<i", 1 << 27) + one[20:], "a_bin_twice": twice,
             "bin_above_the_pseudo_bin": one[:12] + struct.pack("<I", 37451) + one[16:],
             "pseudo_bin_with_one_chunk": one[:12] + struct.pack("<I", 37450) + one[16:],
             "n_intv_past_the_file": one[:-20] + struct.pack("<i", 1 << 28) + one[-16:]}
    out = C.c_void_p()
    assert L.lfq_bam_index_parse(np.frombuffer(one, np.uint8).ctypes.data, len(one), C.byref(out)) == 0 and out
    L.lfq_bam_index_free(out)
    for name, raw in cases.items():
        a = np.frombuffer(raw + b"\0", np.uint8)
        out = C.c_void_p(1)
        assert L.lfq_bam_index_parse(a.ctypes.data, len(raw), C.byref(out)) == LFQ_ERR_INVALID and not out, name
    a = np.frombuffer(good, np.uint8)
    assert L.lfq_bam_index_parse(None, 8, C.byref(out)) == LFQ_ERR_INVALID
    assert L.lfq_bam_index_parse(a.ctypes.data, -1, C.byref(out)) == LFQ_ERR_INVALID
    assert L.lfq_bam_index_parse(a.ctypes.data, len(a), None) == LFQ_ERR_INVALID
    # without the trailing n_no_coor (older writers): 0
    out = C.c_void_p()
    assert L.lfq_bam_index_parse(a.ctypes.data, len(a) - 8, C.byref(out)) == 0
    p, n = C.c_void_p(), C.c_int64()
    assert L.lfq_bam_index_bytes(out, C.byref(p), C.byref(n)) == 0 and C.string_at(p, n.value) == good[:-8] + bytes(8)
    L.lfq_bam_index_free(out)
    L.lfq_bam_index_free(None)


def test_query_and_bytes_refuse_bad_arguments():
    import lofreq_amd as la
    from lofreq_amd import _lib
    L = _lib.load()
    idx = la.BamIndex.from_bytes(load("python").bai)
    b, e, n, p = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_void_p()
    assert L.lfq_bam_index_query(None, 0, 0, 10, C.byref(b), C.byref(e), C.byref(n)) == LFQ_ERR_INVALID
    for tid in (-1, 5):
        assert L.lfq_bam_index_query(idx.h, tid, 0, 10, C.byref(b), C.byref(e), C.byref(n)) == LFQ_ERR_INVALID
    assert L.lfq_bam_index_query(idx.h, 0, 0, 10, None, C.byref(e), C.byref(n)) == LFQ_ERR_INVALID
    assert L.lfq_bam_index_query(idx.h, 0, 0, 10, C.byref(b), None, C.byref(n)) == LFQ_ERR_INVALID
    assert L.lfq_bam_index_query(idx.h, 0, 0, 10, C.byref(b), C.byref(e), None) == LFQ_ERR_INVALID
    assert L.lfq_bam_index_bytes(None, C.byref(p), C.byref(n)) == LFQ_ERR_INVALID
    assert L.lfq_bam_index_bytes(idx.h, None, C.byref(n)) == LFQ_ERR_INVALID
    assert L.lfq_bam_index_bytes(idx.h, C.byref(p), None) == LFQ_ERR_INVALID
    idx.close()


def test_build_and_times_refuse_a_null_context():
    """a NULL context is refused like every other NULL argument.  (The table's rows that an argument check refuses need a context to
    be told apart from this one: tests/test_gpu_bam_index.py runs them.)"""
    from lofreq_amd import _lib
    L = _lib.load()
    row = next(r for r in be.ROWS if r.name == "one_record")
    body = np.frombuffer(row.body, np.uint8)
    ro, do, co = (np.asarray(x, np.int64) for x in (row.rec_off, row.data_off, row.comp_off))
    out = C.c_void_p(1)
    assert L.lfq_bam_index_build(None, body.ctypes.data, len(body), ro.ctypes.data, 1, do.ctypes.data, co.ctypes.data, 1, 0, 2,
                                 C.byref(out)) == LFQ_ERR_INVALID and not out
    t = _lib.BamIndexTimes()
    assert L.lfq_last_bam_index_times(None, C.byref(t)) == LFQ_ERR_INVALID
