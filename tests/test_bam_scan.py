"""lfq_bam_scan_records (host only): the records of inflated BAM bytes, kept as sam_itr_next + mplp_func (plp.c:606-722) keep them,
against a restatement of those rules in Python.  Streams are built from tests/bam_records.py reads with block_size and core in
front (bgzf_edges.bam_record).  No GPU."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import bam_records as br
import bgzf_edges as be

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_MASK = 4 | 256 | 512 | 1024
REF_OPS = "MDN=X"


def _read(l=20, pos0=100, cigar=None, mapq=40, flag=0, seed=0):
    r = br.mk(l, seed, pos0=pos0, tags=None)
    r["mapq"], r["flag_other"], r["reverse"] = mapq, flag & ~16, bool(flag & 16)
    if cigar is not None:
        r["cigar"] = cigar
    return r


def _stream(items):
    """items: (read, ref_id) -> (bytes, [offset of each record])"""
    out, offs = b"", []
    for r, tid in items:
        offs.append(len(out))
        out += be.bam_record(r, tid)
    return out, offs


def _model(items, tid=-1, beg=0, end=2 ** 63 - 1, min_mq=0, max_mq=255, no_orphan=False, flag_mask=DEFAULT_MASK):
    """-> [(index, mapq handed out)] of the kept records"""
    kept = []
    for i, (r, ref_id) in enumerate(items):
        flag = (16 if r.get("reverse") else 0) | r.get("flag_other", 0)
        if ref_id < 0 or (tid >= 0 and ref_id != tid) or (flag & flag_mask):
            continue
        ref_bases = sum(n for op, n in r["cigar"] if op in REF_OPS)
        endpos = r["pos0"] + (ref_bases or 1)
        if not (r["pos0"] < end and endpos > beg):
            continue
        mq = r["mapq"]
        if mq > max_mq:
            mq = max_mq
        elif mq < min_mq:
            continue
        elif no_orphan and (flag & 1) and not (flag & 2):
            continue
        if len(r["qual"]) == 0 or len(r["cigar"]) == 0:
            continue
        kept.append((i, mq))
    return kept


def _check(items, **opts):
    import lofreq_amd as la
    data, offs = _stream(items)
    s = la.bam_scan_records(data, 0, None, **opts)
    want = _model(items, **opts)
    assert s["n_seen"] == len(items) and s["n_consumed"] == len(data)
    assert len(s["pos"]) == len(want), (len(s["pos"]), want)
    ends = offs[1:] + [len(data)]
    for k, (i, mq) in enumerate(want):
        r = items[i][0]
        lq, nc, ls, body = br.record_fields(r)
        assert s["data_off"][k] == offs[i] + 36 and s["data_end"][k] == ends[i]
        assert data[s["data_off"][k]:s["data_end"][k]] == body
        assert (s["pos"][k], s["mapq"][k], s["l_qname"][k], s["n_cigar"][k], s["l_qseq"][k]) == (r["pos0"], mq, lq, nc, ls)
        assert s["flag"][k] == ((16 if r.get("reverse") else 0) | r.get("flag_other", 0))
    assert s["data_off"][-1] == (ends[want[-1][0]] if want else 0)
    return [i for i, _ in want]


def test_every_flag_bit_of_the_mask():
    items = [(_read(flag=1 << b, seed=b), 0) for b in range(12)] + [(_read(flag=0), 0)]
    kept = _check(items)
    assert kept == [b for b in range(12) if not ((1 << b) & DEFAULT_MASK)] + [12]
    for b in range(12):                             # a mask of one bit drops exactly the reads with it
        assert _check(items, flag_mask=1 << b) == [i for i in range(13) if i != b]
    assert len(_check(items, flag_mask=0)) == 13


def test_tid_any_equal_other_and_unplaced():
    items = [(_read(seed=1), 0), (_read(seed=2), 1), (_read(seed=3), -1), (_read(seed=4), 2), (_read(seed=5), 1)]
    assert _check(items) == [0, 1, 3, 4]            # any: all but refID -1
    assert _check(items, tid=1) == [1, 4]
    assert _check(items, tid=7) == []


def test_region_edges_and_endpos():
    items = [(_read(l=20, pos0=80), 0),             # ends exactly at beg = 100: out
             (_read(l=20, pos0=81), 0),             # one base inside
             (_read(l=20, pos0=199), 0),            # starts on the last position
             (_read(l=20, pos0=200), 0),            # starts exactly at end: out
             (_read(l=20, pos0=99, cigar=[("S", 10), ("I", 10)]), 0),      # no reference bases: endpos = pos + 1 = beg: out
             (_read(l=20, pos0=100, cigar=[("S", 10), ("I", 10)]), 0),     # ... endpos 101: in
             (_read(l=20, pos0=60, cigar=[("M", 10), ("D", 25), ("M", 10)]), 0),   # the deletion carries it to 105: in
             (_read(l=20, pos0=60, cigar=[("M", 10), ("N", 20), ("=", 5), ("X", 5)]), 0),   # ends at 100: out
             (_read(l=20, pos0=70, cigar=[("H", 5), ("M", 20), ("P", 3), ("S", 0)]), 0)]    # 90: out
    assert _check(items, beg=100, end=200) == [1, 2, 5, 6]
    assert _check(items) == list(range(9))


def test_mapq_cap_floor_and_the_else_if_order():
    orphan = 1                                      # paired, not proper
    items = [(_read(mapq=10), 0), (_read(mapq=20), 0), (_read(mapq=30), 0), (_read(mapq=50), 0),
             (_read(mapq=50, flag=orphan), 0),      # above the cap: capped, and the orphan test is never reached
             (_read(mapq=30, flag=orphan), 0),      # within: the orphan test drops it
             (_read(mapq=30, flag=1 | 2), 0),       # a proper pair stays
             (_read(mapq=10, flag=orphan), 0)]
    assert _check(items, min_mq=20, max_mq=40) == [1, 2, 3, 4, 5, 6]
    assert _check(items, min_mq=20, max_mq=40, no_orphan=True) == [1, 2, 3, 4, 6]
    assert _check(items, no_orphan=True) == [0, 1, 2, 3, 6]
    assert _check(items, min_mq=20, max_mq=15) == [0 + 1, 2, 3, 4, 5, 6]     # a cap below the floor: the capped ones stay (else if)
    import lofreq_amd as la
    s = la.bam_scan_records(_stream(items)[0], 0, None, min_mq=20, max_mq=40)
    assert s["mapq"].tolist() == [20, 30, 40, 40, 30, 30]


def test_reads_without_bases_or_cigar_are_dropped():
    empty = _read(l=20)
    empty.update(seq=np.zeros(0, np.uint8), qual=np.zeros(0, np.uint8), cigar=[("M", 20)])
    nocig = _read(l=20)
    nocig["cigar"] = []
    items = [(_read(seed=1), 0), (empty, 0), (nocig, 0), (_read(seed=2), 0)]
    assert _check(items) == [0, 3]


def test_a_stream_may_end_anywhere():
    import lofreq_amd as la
    items = [(_read(seed=i, l=10 + i), 0) for i in range(4)]
    data, offs = _stream(items)
    ends = offs[1:] + [len(data)]
    for stop, n, consumed in [(ends[1], 2, ends[1]),             # exactly at a record's end
                              (ends[1] + 2, 2, ends[1]),         # inside block_size
                              (ends[1] + 4, 2, ends[1]),         # block_size alone
                              (ends[1] + 20, 2, ends[1]),        # inside the core
                              (ends[2] - 1, 2, ends[1]),         # inside the record
                              (len(data), 4, len(data)), (0, 0, 0)]:
        s = la.bam_scan_records(data, 0, stop)
        assert (len(s["pos"]), s["n_seen"], s["n_consumed"]) == (n, n, consumed), stop
    s = la.bam_scan_records(data, offs[2], None)                 # first inside the stream
    assert s["n_seen"] == 2 and s["data_off"][0] == offs[2] + 36
    s = la.bam_scan_records(data, offs[1], offs[1])
    assert s["n_seen"] == 0 and s["n_consumed"] == offs[1] and s["data_off"].tolist() == [offs[1]]


def test_invalid_streams_are_refused():
    import lofreq_amd as la
    good = be.bam_record(_read(seed=1), 0)
    short = struct.pack("<i", 31) + good[4:]
    neg = struct.pack("<i", -5) + good[4:]
    long_name = bytearray(good)
    long_name[4 + 8] = 255                          # l_read_name beyond the record
    many_cig = bytearray(good)
    many_cig[4 + 12:4 + 14] = struct.pack("<H", 4000)
    long_seq = bytearray(good)
    long_seq[4 + 16:4 + 20] = struct.pack("<i", 10 ** 6)
    neg_seq = bytearray(good)
    neg_seq[4 + 16:4 + 20] = struct.pack("<i", -1)
    for bad in (short, neg, bytes(long_name), bytes(many_cig), bytes(long_seq), bytes(neg_seq)):
        with pytest.raises(RuntimeError, match="lfq_bam_scan_records"):
            la.bam_scan_records(good + bad)
    for first, stop in ((-1, None), (5, 4)):
        with pytest.raises(RuntimeError):
            la.bam_scan_records(good, first, stop)
    assert la.bam_scan_records(good)["n_seen"] == 1


def test_names_are_declared_bound_and_exported_and_null_is_refused():
    import lofreq_amd as la
    from lofreq_amd import _lib, pileup
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    names = ["lfq_bgzf_inflate", "lfq_last_bgzf_times", "lfq_bam_scan_opts_init", "lfq_bam_scan_records", "lfq_bam_scan_free",
             "lfq_readset_create_from_bgzf"]
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.EXPORTS and getattr(L, n).argtypes is not None, n
    for n in ("bgzf_inflate", "bam_scan_records", "last_bgzf_times", "BgzfError"):
        assert n in la.__all__ and hasattr(la, n)
    assert callable(pileup.ReadSet.from_bgzf)
    assert int(re.search(r"#define LFQ_ABI_VERSION (\d+)", hdr).group(1)) == 10 == L.lfq_abi_version()
    o = _lib.BamScanOpts()
    L.lfq_bam_scan_opts_init(C.byref(o))
    assert (o.tid, o.beg, o.end, o.min_mq, o.max_mq, o.no_orphan, o.flag_mask) == (-1, 0, 2 ** 63 - 1, 0, 255, 0, DEFAULT_MASK)
    L.lfq_bam_scan_opts_init(None)
    L.lfq_bam_scan_free(None)
    inval = -1
    buf = (C.c_uint8 * 64)()
    out = C.POINTER(_lib.BamScan)()
    assert L.lfq_bam_scan_records(None, 0, 0, C.byref(o), C.byref(out)) == inval
    assert L.lfq_bam_scan_records(buf, 0, 0, None, C.byref(out)) == inval
    assert L.lfq_bam_scan_records(buf, 0, 0, C.byref(o), None) == inval
    # without a context nothing of the device entries runs: refused before a device is touched
    res = C.POINTER(_lib.BgzfResult)()
    assert L.lfq_bgzf_inflate(None, buf, 0, C.byref(res)) == inval
    assert L.lfq_last_bgzf_times(None, None) == inval
    h = C.c_void_p()
    assert L.lfq_readset_create_from_bgzf(None, buf, 0, 0, -1, C.byref(o), C.cast(C.c_char_p(b"ACGT"), C.c_void_p), 4, 0,
                                          C.byref(h), None) == inval
