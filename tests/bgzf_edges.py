"""Raw deflate streams and their BGZF framing, for the tests of lfq_inflate.h and lfq_bgzf_inflate.

ROWS            one Row per stream: name, payload (None: no decoder accepts the stream), raw deflate bytes, verdict:
                  "ok"       zlib.decompress(raw, -15) == payload, and so must every decoder of this project
                  "deflate"  zlib raises; the block's status is nonzero
                  "trailer"  the stream is fine and decodes to payload, but the block's trailer (isize / crc of the Row) is not its
                             own: the status is nonzero
                isize / crc: what the block's trailer says when that is not len(payload) / crc32(payload); a "deflate" row is given
                room (4096) so that the decoder meets the defect itself and not the end of the output first
                frameable: False for the one row whose stream does not fit a BGZF block (BSIZE is 16 bits: 65536 bytes, header
                and trailer included) -- it runs on the host only
FRAMING_BAD     name -> bytes that lfq_bgzf_inflate refuses before a device is touched
bgzf_block()    one BGZF block around a raw stream (SAM specification section 4.1)
Most rows come from zlib.compressobj(level, DEFLATED, -15, 9, strategy); a small bit writer builds the rest.  No test in here."""
import collections
import struct
import zlib

import numpy as np

Row = collections.namedtuple("Row", "name payload raw verdict isize crc frameable")


def _row(name, payload, raw, verdict="ok", isize=None, crc=None, frameable=True):
    if verdict == "deflate" and isize is None:
        isize = 4096        # room enough that the decoder meets the defect itself and not the end of the output first
    return Row(name, payload, bytes(raw), verdict, isize, crc, frameable)


def bgzf_block(raw, payload=b"", isize=None, crc=None, extra_before=b"", extra_after=b"", bsize=None):
    """header (ID 31 139, CM 8, FLG 4, XLEN, the BC subfield among the extra subfields) | raw | CRC32 | ISIZE"""
    xlen = len(extra_before) + 6 + len(extra_after)
    total = 12 + xlen + len(raw) + 8
    assert total <= 65536 or bsize is not None, total
    head = struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, xlen) + extra_before
    head += b"BC" + struct.pack("<HH", 2, (total - 1 if bsize is None else bsize) & 0xffff) + extra_after
    return head + bytes(raw) + struct.pack("<II", zlib.crc32(payload) if crc is None else crc, len(payload) if isize is None else isize)


def frame(row):
    """the Row as one BGZF block"""
    return bgzf_block(row.raw, row.payload or b"", row.isize, row.crc)


EOF_BLOCK = bgzf_block(b"\x03\x00")     # the 28-byte end-of-file marker


def bam_record(r, ref_id=0, **kw):
    """one record as it lies in a BAM file: block_size, the 32-byte core, then what bam_records.record_fields makes of the read
    dict r (flag: 16 for r["reverse"] | r["flag_other"]); kw goes to record_fields"""
    import bam_records as br
    l_qname, n_cigar, l_qseq, data = br.record_fields(r, **kw)
    flag = (16 if r.get("reverse") else 0) | (r.get("flag_other", 0) & ~16)
    core = struct.pack("<iiBBHHHiiii", ref_id, r["pos0"], l_qname, r.get("mapq", 60), 4680, n_cigar, flag, l_qseq, -1, -1, 0)
    return struct.pack("<i", len(core) + len(data)) + core + data


def bgzf_blocks(payload, cuts, level=6):
    """payload cut at the offsets `cuts` into BGZF blocks (each piece at most 65280 bytes)"""
    out, edges = b"", [0] + list(cuts) + [len(payload)]
    for a, b in zip(edges[:-1], edges[1:]):
        assert 0 <= b - a <= 65280
        out += bgzf_block(deflate(payload[a:b], level), payload[a:b])
    return out


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, flush=zlib.Z_FULL_FLUSH):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        return co.compress(data) + co.flush()
    return co.compress(data[:flush_at]) + co.flush(flush) + co.compress(data[flush_at:]) + co.flush()


# ---- the bit writer --------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):
        """n bits of v, least significant first (header fields, extra bits)"""
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, c):
        """a Huffman code (value, length), most significant bit first"""
        v, n = c
        for k in range(n - 1, -1, -1):
            self.bits((v >> k) & 1, 1)
        return self

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return self

    def raw(self, b):
        assert self.n == 0
        self.out += bytes(b)
        return self

    def done(self):
        return bytes(self.align().out)


def canon(lens):
    """symbol -> (code, length) of the canonical code with these lengths (RFC 1951 section 3.2.2)"""
    out, code = {}, 0
    for L in range(1, 16):
        for s, l in enumerate(lens):
            if l == L:
                out[s] = (code, L)
                code += 1
        code <<= 1
    return out


def fixed_lit(s):
    if s < 144:
        return (0x30 + s, 8)
    if s < 256:
        return (0x190 + s - 144, 9)
    if s < 280:
        return (s - 256, 7)
    return (0xc0 + s - 280, 8)


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577]
DEXT = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]


def put_match(w, lit_code, dist_code, length, dist):
    ls = max(i for i in range(29) if LBASE[i] <= length and (i == 28 or length < 258))
    w.code(lit_code(257 + ls)).bits(length - LBASE[ls], LEXT[ls])
    ds = max(i for i in range(30) if DBASE[i] <= dist)
    w.code(dist_code(ds)).bits(dist - DBASE[ds], DEXT[ds])


def stored_block(w, data, final, nlen=None):
    w.bits(final, 1).bits(0, 2).align()
    w.raw(struct.pack("<HH", len(data), (~len(data) & 0xffff) if nlen is None else nlen)).raw(data)
    return w


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def flat_lengths(k):
    """lengths of a complete code over k >= 2 symbols"""
    m = max(1, (k - 1).bit_length())
    short = (1 << m) - k
    return [m - 1] * short + [m] * (k - short)


def dyn_header(w, final, nlen, ndist, ops, cl_lens=None):
    """BFINAL, BTYPE 2, HLIT, HDIST, HCLEN 19, the code-length code, then the ops: a length 0..15, or (16 | 17 | 18, repeat count).
    cl_lens: the 19 lengths of the code-length code; None = a complete code over the symbols the ops use (two at least)"""
    used = sorted({o if isinstance(o, int) else o[0] for o in ops})
    if cl_lens is None:
        if len(used) == 1:
            used = sorted(set(used) | {0 if used[0] else 1})
        cl_lens = [0] * 19
        for s, l in zip(used, flat_lengths(len(used))):
            cl_lens[s] = l
    cc = canon(cl_lens)
    w.bits(final, 1).bits(2, 2).bits(nlen - 257, 5).bits(ndist - 1, 5).bits(15, 4)
    for s in CL_ORDER:
        w.bits(cl_lens[s], 3)
    for o in ops:
        if isinstance(o, int):
            w.code(cc[o])
        else:
            s, rep = o
            w.code(cc[s]).bits(rep - (11 if s == 18 else 3), 2 if s == 16 else 3 if s == 17 else 7)
    return w


def plain_ops(lens):
    """every length as itself, runs of zeros as 17 / 18"""
    ops, i = [], 0
    while i < len(lens):
        if lens[i] == 0:
            j = i
            while j < len(lens) and lens[j] == 0 and j - i < 138:
                j += 1
            if j - i >= 11:
                ops.append((18, j - i))
            elif j - i >= 3:
                ops.append((17, j - i))
            else:
                ops += [0] * (j - i)
            i = j
        else:
            ops.append(lens[i])
            i += 1
    return ops


def expand_ops(ops):
    out = []
    for o in ops:
        if isinstance(o, int):
            out.append(o)
        else:
            out += [out[-1] if o[0] == 16 else 0] * o[1]
    return out


def dyn_block(ll, dl, body, final=1, ops=None, cl_lens=None):
    """a dynamic block: ll / dl = dicts symbol -> length; body(w, lit_code, dist_code) writes the symbols (end-of-block included)"""
    nlen = max(257, max(ll) + 1)
    ndist = max(1, max(dl) + 1) if dl else 1
    lens = [ll.get(s, 0) for s in range(nlen)] + [dl.get(s, 0) for s in range(ndist)]
    if ops is None:
        ops = plain_ops(lens)
    else:
        assert expand_ops(ops) == lens, (expand_ops(ops), lens)
    w = dyn_header(Bits(), final, nlen, ndist, ops, cl_lens)
    lc, dc = canon(lens[:nlen]), canon(lens[nlen:])
    body(w, lambda s: lc[s], lambda s: dc[s])
    return w.done()


def _payload(n, seed=1):
    """compressible and not trivial: words of a small vocabulary with noise"""
    rng = np.random.default_rng(seed)
    if n == 0:
        return b""
    words = [bytes(rng.integers(65, 91, int(k)).astype(np.uint8)) for k in rng.integers(2, 12, 40)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, 40))]
        if rng.random() < 0.2:
            out += bytes(rng.integers(0, 256, 3).astype(np.uint8))
    return bytes(out[:n])


def _rows():
    R = []
    text = _payload(3000)
    # ---- stored
    R.append(_row("stored_level0", text, deflate(text, 0)))
    R.append(_row("stored_empty_from_sync_flush", text, deflate(text, 6, flush_at=1500, flush=zlib.Z_SYNC_FLUSH)))
    big = _payload(65535, 2)
    R.append(_row("stored_65535", big, stored_block(Bits(), big, 1).done(), frameable=False))
    # ---- fixed, dynamic
    R.append(_row("fixed", text, deflate(text, 6, zlib.Z_FIXED)))
    for lv in (1, 6, 9):
        R.append(_row("dynamic_level%d" % lv, text, deflate(text, lv)))
    R.append(_row("huffman_only", text, deflate(text, 6, zlib.Z_HUFFMAN_ONLY)))
    rle = b"".join(bytes([65 + i % 7]) * (300 + 17 * i) for i in range(12))
    R.append(_row("rle_distance1_length258", rle, deflate(rle, 6, zlib.Z_RLE)))
    mixed = text + bytes(np.random.default_rng(3).integers(0, 256, 700).astype(np.uint8)) + b"A" * 900
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    raw = co.compress(mixed[:1000]) + co.flush(zlib.Z_FULL_FLUSH)
    co2 = zlib.compressobj(0, zlib.DEFLATED, -15)
    # (three members' blocks in one stream: each but the last ends at a byte boundary behind a full flush)
    raw += co2.compress(mixed[1000:2000]) + co2.flush(zlib.Z_FULL_FLUSH) + deflate(mixed[2000:], 9)
    R.append(_row("blocks_of_three_types", mixed, raw))
    R.append(_row("full_flush_midway", text, deflate(text, 6, flush_at=1234)))
    # ---- sizes
    for n in (0, 1, 65280, 65536):
        p = _payload(n, 10 + n % 7)
        R.append(_row("size_%d" % n, p, deflate(p, 6)))
    # ---- hand-built, well-formed
    far = _payload(32768, 4)
    w = stored_block(Bits(), far, 0)
    w.bits(1, 1).bits(1, 2)
    put_match(w, fixed_lit, lambda s: (s, 5), 10, 32768)
    w.code(fixed_lit(256))
    R.append(_row("distance_32768", far + far[:10], w.done()))
    # a 15-bit code: 'a' 1 bit, end-of-block 2, bytes 0..11 3..14 bits, bytes 12 and 13 15 bits; no distance code
    ll15 = {97: 1, 256: 2, 12: 15, 13: 15}
    ll15.update({b: 3 + b for b in range(12)})
    p15 = b"aa" + bytes(range(14)) + b"a" + bytes([13, 12, 13, 0])

    def lits(p):
        def body(w, lc, dc):
            for b in p:
                w.code(lc(b))
            w.code(lc(256))
        return body
    R.append(_row("code_of_15_bits", p15, dyn_block(ll15, {}, lits(p15))))
    # all 19 code-length symbols in use: lengths 1 .. 15, a single 0, 17, 18, and 16 over four distance lengths of 2; length symbol
    # 257 takes the place of byte 13 among the 15-bit codes
    ll19 = dict(ll15)
    del ll19[13]
    ll19[257] = 15
    ops19 = list(range(3, 15)) + [15, 0, 0, (17, 3), (18, 79), 1, (18, 138), (18, 20), 2, 15, 2, (16, 3)]
    assert {o if isinstance(o, int) else o[0] for o in ops19} == set(range(19))
    p19 = b"aa" + bytes(range(13)) + b"a"

    def body19b(w, lc, dc):
        for b in p19:
            w.code(lc(b))
        for d in (1, 2, 3, 4):
            put_match(w, lc, dc, 3, d)
        w.code(lc(256))
    out19 = bytearray(p19)
    for d in (1, 2, 3, 4):
        for _ in range(3):
            out19.append(out19[-d])
    R.append(_row("all_19_code_length_codes", bytes(out19), dyn_block(ll19, {0: 2, 1: 2, 2: 2, 3: 2}, body19b, ops=ops19)))
    # a 16-repeat that starts at literal/length 256 and runs on over the four distance lengths
    llx = {97: 1, 255: 2, 256: 2}
    opsx = [(18, 97), 1, (18, 138), (18, 19), 2, (16, 5)]

    def bodyx(w, lc, dc):
        for b in b"a\xffaa":
            w.code(lc(b))
        w.code(lc(256))
    R.append(_row("repeat_crosses_into_distance_lengths", b"a\xffaa", dyn_block(llx, {0: 2, 1: 2, 2: 2, 3: 2}, bodyx, ops=opsx)))
    # one distance code of one bit: the incomplete set zlib allows
    ll1 = {97: 1, 256: 2, 257: 2}

    def body1(w, lc, dc):
        w.code(lc(97))
        put_match(w, lc, dc, 3, 1)
        w.code(lc(256))
    R.append(_row("single_distance_code_of_1_bit", b"aaaa", dyn_block(ll1, {0: 1}, body1)))
    # ---- malformed deflate
    R.append(_row("block_type_3", None, Bits().bits(1, 1).bits(3, 2).done(), "deflate"))
    R.append(_row("stored_len_not_nlen", None, stored_block(Bits(), b"abcd", 1, nlen=0x1234).done(), "deflate"))
    eob = lambda w, lc, dc: w.code(lc(256))
    nothing = lambda w, lc, dc: w
    R.append(_row("repeat_16_at_the_first_length", None,
                  dyn_header(Bits(), 1, 257, 1, [(16, 3), (18, 138), (18, 115), 1, 1], None).bits(0, 16).done(), "deflate"))
    w = dyn_header(Bits(), 1, 257, 1, plain_ops([0] * 97 + [1, 1] + [0] * 157 + [1, 0]))
    R.append(_row("oversubscribed_set", None, w.bits(0, 16).done(), "deflate"))
    w = dyn_header(Bits(), 1, 257, 1, plain_ops([0] * 97 + [2] + [0] * 158 + [2, 0]))
    R.append(_row("incomplete_literal_length_set", None, w.bits(0, 16).done(), "deflate"))
    w = dyn_header(Bits(), 1, 257, 1, plain_ops([0] * 97 + [1, 1] + [0] * 157 + [0, 0]))
    R.append(_row("no_end_of_block_code", None, w.bits(0, 16).done(), "deflate"))
    w = dyn_header(Bits(), 1, 257, 1, [1] * 258, cl_lens=[1, 1, 1] + [0] * 16)
    R.append(_row("oversubscribed_code_length_code", None, w.bits(0, 16).done(), "deflate"))
    for s in (286, 287):
        w = Bits().bits(1, 1).bits(1, 2).code(fixed_lit(97)).code(fixed_lit(s)).bits(0, 5).bits(0, 7)
        R.append(_row("length_symbol_%d" % s, None, w.bits(0, 16).done(), "deflate"))
    for s in (30, 31):
        w = Bits().bits(1, 1).bits(1, 2).code(fixed_lit(97)).code(fixed_lit(257)).code((s, 5)).code(fixed_lit(256))
        R.append(_row("distance_symbol_%d" % s, None, w.bits(0, 16).done(), "deflate"))
    w = Bits().bits(1, 1).bits(1, 2).code(fixed_lit(97))
    put_match(w, fixed_lit, lambda s: (s, 5), 3, 2)
    R.append(_row("distance_before_the_output", None, w.code(fixed_lit(256)).done(), "deflate"))
    fx = deflate(text, 6, zlib.Z_FIXED)
    R.append(_row("input_ends_inside_a_symbol", None, fx[:len(fx) // 2], "deflate"))
    R.append(_row("input_ends_inside_a_dynamic_header", None, deflate(text, 6)[:20], "deflate"))
    R.append(_row("input_ends_inside_a_stored_block", None, stored_block(Bits(), b"x" * 100, 1).done()[:55], "deflate"))
    R.append(_row("input_ends_inside_a_stored_header", None, stored_block(Bits(), b"x" * 100, 1).done()[:3], "deflate"))
    R.append(_row("empty_input", None, b"", "deflate"))
    # ---- the trailer is not the stream's
    tail = b"abcabcabc" * 20
    w = Bits().bits(1, 1).bits(1, 2)
    for b in b"abc":
        w.code(fixed_lit(b))
    put_match(w, fixed_lit, lambda s: (s, 5), len(tail) - 3, 3)
    raw_tail = w.code(fixed_lit(256)).done()
    R.append(_row("match_runs_one_byte_past_isize", tail, raw_tail, "trailer", isize=len(tail) - 1))
    R.append(_row("literal_one_byte_past_isize", text, deflate(text, 6, zlib.Z_HUFFMAN_ONLY), "trailer", isize=len(text) - 1))
    R.append(_row("stored_one_byte_past_isize", text, deflate(text, 0), "trailer", isize=len(text) - 1))
    R.append(_row("one_byte_short_of_isize", text, deflate(text, 6), "trailer", isize=len(text) + 1))
    R.append(_row("wrong_isize", text, deflate(text, 6), "trailer", isize=len(text) // 2))
    R.append(_row("wrong_crc", text, deflate(text, 6), "trailer", crc=zlib.crc32(text) ^ 0x100))
    names = [r.name for r in R]
    assert len(set(names)) == len(names)
    return R


ROWS = _rows()

_good = bgzf_block(deflate(b"hello, bgzf"), b"hello, bgzf")
_no_bc = struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, 6) + b"XY" + struct.pack("<HH", 2, 0) + deflate(b"") + struct.pack("<II", 0, 0)
FRAMING_BAD = {
    "bad_magic": b"\x1f\x8c" + _good[2:],
    "cm_not_8": _good[:2] + b"\x07" + _good[3:],
    "no_fextra": _good[:3] + b"\x00" + _good[4:],
    "no_bc_subfield": _no_bc,
    "bc_of_length_3": _good[:14] + struct.pack("<H", 3) + _good[16:],
    "subfield_runs_past_xlen": _good[:10] + struct.pack("<H", 4) + _good[12:],
    "block_shorter_than_header_and_trailer": bgzf_block(deflate(b""), b"", bsize=20),
    "block_runs_past_the_input": _good[:-1],
    "second_block_runs_past_the_input": _good + _good[:30],
    "header_cut": _good + _good[:11],
    "isize_above_65536": bgzf_block(deflate(b"x"), b"x", isize=65537),
}
# an extra subfield in front of (and behind) BC is fine
EXTRA_SUBFIELD_BLOCK = bgzf_block(deflate(b"hello, bgzf"), b"hello, bgzf", extra_before=b"AB" + struct.pack("<H", 3) + b"xyz",
                                  extra_after=b"CD" + struct.pack("<H", 0))
EXTRA_SUBFIELD_PAYLOAD = b"hello, bgzf"
