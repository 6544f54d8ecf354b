"""CPU tests of lfq_bgzf_deflate and lfq_bam_frame_encoded: the symbols and the Python names exist, the arguments refused "before a
device is touched" are refused without one, and the model of core.bin that tests/test_gpu_bgzf_deflate.py holds the kernel to --
reg2bin of the SAM specification, section 5.3 -- agrees with the bin of every record of a BAM that went through htslib
(tests/golden/bgzf_binary.json).  No device."""
import base64
import ctypes as C
import json
import os
import re
import struct

import numpy as np

import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
REF_OPS = (0, 2, 3, 7, 8)       # M D N = X


def reg2bin(beg, end):
    """SAM specification section 5.3: the bin of the zero-based half-open interval [beg, end)"""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def record_bin(pos, flag, cigar_words):
    """core.bin of a record: section 4.2 -- the alignment counts as one base long when it has no reference bases or the read is
    unmapped"""
    ref = sum(int(w) >> 4 for w in cigar_words if int(w) & 15 in REF_OPS)
    return reg2bin(pos, pos + (1 if (flag & 4) or ref == 0 else ref))


def parse_bam_body(data):
    """inflated BAM bytes -> (offset of the first record, [dict(off, block_size, core (32 bytes), pos, l_qname, mapq, bin, n_cigar,
    flag, l_qseq, data = the bytes from read_name on)], l_ref of the first reference)"""
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", data, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, o)
    o += 4
    l_ref0 = 0
    for k in range(n_ref):
        l_name, = struct.unpack_from("<i", data, o)
        l_ref, = struct.unpack_from("<i", data, o + 4 + l_name)
        l_ref0 = l_ref0 or l_ref
        o += 4 + l_name + 4
    first, recs = o, []
    while o < len(data):
        block_size, _ref_id, pos, l_name, mapq, bin_, n_cigar, flag, l_seq = struct.unpack_from("<iiiBBHHHi", data, o)
        recs.append({"off": o, "block_size": block_size, "core": data[o + 4:o + 36], "pos": pos, "l_qname": l_name, "mapq": mapq,
                     "bin": bin_, "n_cigar": n_cigar, "flag": flag, "l_qseq": l_seq, "data": data[o + 36:o + 4 + block_size]})
        o += 4 + block_size
    assert o == len(data)
    return first, recs, l_ref0


def cigar_words(rec):
    return np.frombuffer(rec["data"][rec["l_qname"]:rec["l_qname"] + 4 * rec["n_cigar"]], "<u4")


def test_the_symbols_and_the_python_names_exist():
    import lofreq_amd as la
    from lofreq_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    for n in ("lfq_bgzf_deflate", "lfq_last_bgzf_deflate_times", "lfq_bam_frame_encoded"):
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.EXPORTS and getattr(L, n).argtypes is not None, n
    for n in ("bgzf_deflate", "last_bgzf_deflate_times", "bam_frame_encoded"):
        assert callable(getattr(la, n)) and n in la.__all__, n
    assert la.LFQ_BGZF_PUT_EOF == 1 == int(re.search(r"#define LFQ_BGZF_PUT_EOF (\d+)", hdr).group(1))
    assert C.sizeof(_lib.BgzfDeflated) == 48 and C.sizeof(_lib.BgzfDeflateTimes) == 56 and C.sizeof(_lib.BamFramed) == 32
    assert int(re.search(r"#define LFQ_ABI_VERSION (\d+)", hdr).group(1)) == 10


def test_arguments_refused_before_a_device_is_touched():
    """with a NULL context, and -- every other argument being looked at first -- with memory that is no context at all"""
    from lofreq_amd import _lib
    L = _lib.load()
    out = C.POINTER(_lib.BgzfDeflated)()
    buf = np.zeros(70000, np.uint8)
    not_a_context = np.zeros(1 << 16, np.uint8)         # (all zero: no state of any call hangs off it)
    ctx = not_a_context.ctypes.data
    d = buf.ctypes.data

    def cuts(*v):
        a = np.array(v, np.int64)
        return a, a.ctypes.data, len(v)

    assert L.lfq_bgzf_deflate(None, d, 10, None, 0, 0, C.byref(out)) == INVALID
    assert L.lfq_bgzf_deflate(ctx, d, 10, None, 0, 0, None) == INVALID
    assert L.lfq_bgzf_deflate(ctx, d, -1, None, 0, 0, C.byref(out)) == INVALID
    assert L.lfq_bgzf_deflate(ctx, None, 10, None, 0, 0, C.byref(out)) == INVALID
    assert L.lfq_bgzf_deflate(ctx, d, 10, None, 0, 2, C.byref(out)) == INVALID             # an unknown flag bit
    assert L.lfq_bgzf_deflate(ctx, d, 10, None, 0, 1 | 4, C.byref(out)) == INVALID
    assert L.lfq_bgzf_deflate(ctx, d, 10, None, 1, 0, C.byref(out)) == INVALID             # NULL cuts with n_cuts > 0
    keep, p, n = cuts(5)
    assert L.lfq_bgzf_deflate(ctx, d, 10, p, -1, 0, C.byref(out)) == INVALID
    for bad in ((0,), (10,), (11,), (-3,), (4, 4), (6, 5), (3, 7, 7)):                      # not strictly increasing inside (0, n)
        keep, p, n = cuts(*bad)
        assert L.lfq_bgzf_deflate(ctx, d, 10, p, n, 0, C.byref(out)) == INVALID, bad
    keep, p, n = cuts(100, 100 + 65281)
    assert L.lfq_bgzf_deflate(ctx, d, 70000, p, n, 0, C.byref(out)) == INVALID             # a piece above 65280 bytes
    keep, p, n = cuts(4719)
    assert L.lfq_bgzf_deflate(ctx, d, 70000, p, n, 0, C.byref(out)) == INVALID             # ... the last one
    assert not out
    assert L.lfq_last_bgzf_deflate_times(None, None) == INVALID
    t = _lib.BgzfDeflateTimes()
    assert L.lfq_last_bgzf_deflate_times(None, C.byref(t)) == INVALID
    fr = C.POINTER(_lib.BamFramed)()
    assert L.lfq_bam_frame_encoded(None, d, 1, C.byref(fr)) == INVALID
    assert L.lfq_bam_frame_encoded(ctx, None, 1, C.byref(fr)) == INVALID
    assert L.lfq_bam_frame_encoded(ctx, d, 1, None) == INVALID
    assert L.lfq_bam_frame_encoded(ctx, d, -1, C.byref(fr)) == INVALID
    assert L.lfq_bam_frame_encoded(ctx, d, 1, C.byref(fr)) == INVALID                       # no live encode result
    assert not fr and not not_a_context.any()


def test_reg2bin_agrees_with_the_bins_htslib_wrote():
    fx = json.load(open(os.path.join(gu.GOLDEN_DIR, "bgzf_binary.json")))
    _, recs, _ = parse_bam_body(base64.b64decode(fx["inflated_base64"]))
    assert len(recs) == fx["n_reads"] > 0
    for r in recs:
        assert record_bin(r["pos"], r["flag"], cigar_words(r)) == r["bin"], r["off"]


def test_reg2bin_at_its_edges():
    assert reg2bin(-1, 0) == 4680                       # an unplaced read: pos -1, one base long
    assert reg2bin(0, 1) == 4681 and reg2bin(16383, 16384) == 4681 and reg2bin(16384, 16385) == 4682
    assert reg2bin(16380, 16400) == 585                 # across a 16 kb edge: the 128 kb level
    assert reg2bin(0, 1 << 29) == 0
    assert record_bin(-1, 4, [(50 << 4) | 0]) == 4680 and record_bin(100, 0, [(20 << 4) | 4]) == reg2bin(100, 101)
