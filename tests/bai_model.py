"""The .bai of a BAM as the reference's 2.1.4 binary (`lofreq index`) writes it, restated in Python for the tests of
lfq_bam_index_build: from the bytes of a BGZF file (file_tables + build) or from a body plus block tables (build alone).  Also a
.bai parser, a serialiser, the region query of lfq_bam_index_query and a brute-force "records overlapping a region".

The rules are the seven INTEGRATION.md section 13 lists, in the functions below: record_span (1), voffset (2), build (3, 5),
fill_linear (4), merge_bins (6), to_bytes / parse_bai (7).  tests/golden/bai_binary.json decides, not that list: where the fixture
disagrees with a rule the fixture is right (tests/test_bai_model.py holds this file to it).  This file and the library write bins
in ascending number with 37450 last, the binary in its hash table's order, so files are compared PARSED.

A mapped record with refID >= 0 and pos = -1 (nothing the binary is ever given) has bin 4680 and touches window 0.
No test in here."""
import struct
import zlib

META_BIN = 37450
MAX_END = 1 << 29
LEVEL_FIRST = (0, 1, 9, 73, 585, 4681)
REF_OPS = (0, 2, 3, 7, 8)


class BaiError(Exception):
    """what lfq_bam_index_build refuses; .record = the first bad record (-1: an argument)"""

    def __init__(self, record, why):
        Exception.__init__(self, "record %d: %s" % (record, why))
        self.record = record
        self.why = why


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def reg2bins(beg, end):
    end -= 1
    bins = [0]
    for shift, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins.extend(range(base + (beg >> shift), base + (end >> shift) + 1))
    return bins


def bin_level(b):
    return max(l for l in range(6) if b >= LEVEL_FIRST[l])


# ---- records and files for the fixtures ---------------------------------------------------------------------------------------------

OPS = "MIDNSHP=X"
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def record(ref_id, pos, cigar, flag=0, name=b"r", fill=0, stored_bin=0xbeef, aux=b""):
    """one record as it lies in a BAM body: block_size, core, name, CIGAR [(op letter, length)], sequence and qualities made from
    `fill`, aux.  The stored bin is deliberately not the record's (rule 1 does not read it)."""
    l_seq = sum(ln for op, ln in cigar if op in "MIS=X")
    words = b"".join(struct.pack("<I", (ln << 4) | OPS.index(op)) for op, ln in cigar)
    seq = bytes((0x11 * (1 << ((fill + i) & 3))) & 0xff for i in range((l_seq + 1) // 2))
    qual = bytes(2 + (fill * 7 + i * 13) % 39 for i in range(l_seq))
    rest = name + b"\0" + words + seq + qual + aux
    core = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name) + 1, 30 if ref_id >= 0 else 0, stored_bin, len(cigar), flag, l_seq,
                       -1, -1, 0)
    return struct.pack("<i", 32 + len(rest)) + core + rest


def header(refs, sort_order="coordinate"):
    text = ("@HD\tVN:1.0\tSO:%s\n" % sort_order + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)).encode()
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        out.append(struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", length))
    return b"".join(out)


def bgzf_file(payload, cuts):
    """payload cut at `cuts` into BGZF blocks whose deflate stream is one stored block -- written by hand, so that the file's bytes,
    and with them every virtual offset, depend on no compressor's version --, and the end-of-file marker"""
    out, edges = [], [0] + list(cuts) + [len(payload)]
    for a, b in zip(edges, edges[1:]):
        n = b - a
        assert 0 < n <= 65280
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", n + 5 + 25) + b"\x01"
                   + struct.pack("<HH", n, n ^ 0xffff) + payload[a:b] + struct.pack("<II", zlib.crc32(payload[a:b]), n))
    return b"".join(out) + EOF_BLOCK


# ---- a BGZF file -> the arguments of build ---------------------------------------------------------------------------------------

def file_tables(bam):
    """-> (inflated bytes, data_off, comp_off) of the blocks of a BGZF file; the empty blocks at its end (the end-of-file marker)
    are no blocks of the tables, so that comp_off[n_blocks] is where the marker starts"""
    data, data_off, comp_off, o = [], [0], [0], 0
    while o < len(bam):
        assert bam[o:o + 4] == b"\x1f\x8b\x08\x04"
        xlen, = struct.unpack_from("<H", bam, o + 10)
        p, size = o + 12, None
        while p < o + 12 + xlen:
            si, slen = bam[p:p + 2], struct.unpack_from("<H", bam, p + 2)[0]
            if si == b"BC" and slen == 2:
                size = struct.unpack_from("<H", bam, p + 4)[0] + 1
            p += 4 + slen
        pay = zlib.decompress(bam[o + 12 + xlen:o + size - 8], -15)
        assert struct.unpack_from("<II", bam, o + size - 8) == (zlib.crc32(pay), len(pay))
        data.append(pay)
        data_off.append(data_off[-1] + len(pay))
        o += size
        comp_off.append(o)
    while len(data_off) > 1 and data_off[-1] == data_off[-2]:
        data_off.pop()
        comp_off.pop()
    return b"".join(data), data_off, comp_off


def parse_header(data):
    """-> (offset of the first record, [(name, length)]) of inflated BAM bytes"""
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", data, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, o)
    o += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, o)
        refs.append((data[o + 4:o + 4 + l_name - 1].decode(), struct.unpack_from("<i", data, o + 4 + l_name)[0]))
        o += 8 + l_name
    return o, refs


def record_chain(data, first, stop=None):
    """-> rec_off [n + 1] of the complete records of data[first .. stop)"""
    stop = len(data) if stop is None else stop
    off = [first]
    while off[-1] + 4 <= stop:
        size, = struct.unpack_from("<i", data, off[-1])
        if size < 32:
            raise BaiError(len(off) - 1, "block_size")
        if off[-1] + 4 + size > stop:
            break
        off.append(off[-1] + 4 + size)
    return off


def record_cuts(rec_off, max_piece=65280):
    """INTEGRATION.md section 13's loop: the cuts of a body rec_off[0] .. rec_off[n] into pieces of at most max_piece bytes, each cut
    the last record boundary that keeps the piece that long; a longer record is cut every max_piece bytes"""
    cuts, start, j, n = [], rec_off[0], 1, len(rec_off) - 1
    end = rec_off[n]
    while end - start > max_piece:
        while j <= n and rec_off[j] - start <= max_piece:
            j += 1
        cut = rec_off[j - 1] if rec_off[j - 1] > start else start + max_piece
        cuts.append(cut)
        start = cut
    return cuts


# ---- rules 1 - 3, 5: the record pass -----------------------------------------------------------------------------------------------

def record_fields(body, o):
    size, ref_id, pos, l_name, _mapq, _bin, n_cigar, flag, _l_seq = struct.unpack_from("<iiiBBHHHi", body, o)
    return size, ref_id, pos, l_name, n_cigar, flag


def record_span(body, o):
    """-> (refID, beg, end, mapped) of the record at o (rule 1)"""
    _size, ref_id, pos, l_name, n_cigar, flag = record_fields(body, o)
    words = struct.unpack_from("<%dI" % n_cigar, body, o + 36 + l_name)
    rlen = sum(w >> 4 for w in words if (w & 15) in REF_OPS)
    end = pos + 1 if rlen == 0 or flag & 4 else pos + rlen
    return ref_id, pos, end, not flag & 4


def voffset(p, data_off, comp_off, file_off=0):
    nb = len(data_off) - 1
    if p >= data_off[nb]:
        return (comp_off[nb] + file_off) << 16
    lo, hi = 0, nb - 1                              # the last block that starts at or in front of p
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if data_off[mid] <= p:
            lo = mid
        else:
            hi = mid - 1
    return ((comp_off[lo] + file_off) << 16) | (p - data_off[lo])


def check_arguments(body_len, rec_off, data_off, comp_off, n_ref):
    if n_ref < 0 or len(rec_off) < 1 or len(data_off) < 1 or len(data_off) != len(comp_off):
        raise BaiError(-1, "counts")
    for name, off in (("rec_off", rec_off), ("data_off", data_off), ("comp_off", comp_off)):
        strict = name != "data_off"
        for a, b in zip(off, off[1:]):
            if b < a or (strict and b == a):
                raise BaiError(-1, name + " not increasing")
    if rec_off[0] < data_off[0] or rec_off[-1] > data_off[-1] or rec_off[0] < 0 or rec_off[-1] > body_len or comp_off[0] < 0:
        raise BaiError(-1, "records outside the blocks")


def check_record(body, rec_off, j, n_ref):
    """the per-record refusals, each from record j and the core of record j - 1 alone; -> None or the reason"""
    o, length = rec_off[j], rec_off[j + 1] - rec_off[j]
    if length < 36 or struct.unpack_from("<i", body, o)[0] + 4 != length:
        return "block_size"
    _size, ref_id, pos, l_name, n_cigar, _flag = record_fields(body, o)
    if l_name + 4 * n_cigar > length - 36:
        return "name and CIGAR"
    if ref_id >= n_ref or ref_id < -1:
        return "refID"
    if ref_id >= 0 and (pos < -1 or record_span(body, o)[2] > MAX_END):
        return "pos"
    if j > 0 and rec_off[j] - rec_off[j - 1] >= 36:
        p_ref, p_pos = struct.unpack_from("<ii", body, rec_off[j - 1] + 4)
        if ref_id >= 0 and (p_ref < 0 or ref_id < p_ref or (ref_id == p_ref and pos < p_pos)):
            return "order"
    return None


def record_pass(body, rec_off, data_off, comp_off, file_off, n_ref):
    """-> [(refID, bin, u, v, mapped, first window, last window)] per record, or BaiError with the first bad record"""
    out = []
    for j in range(len(rec_off) - 1):
        why = check_record(body, rec_off, j, n_ref)
        if why:
            raise BaiError(j, why)
        ref_id, beg, end, mapped = record_span(body, rec_off[j])
        u = voffset(rec_off[j], data_off, comp_off, file_off)
        v = voffset(rec_off[j + 1], data_off, comp_off, file_off)
        out.append((ref_id, reg2bin(beg, end), u, v, mapped, max(beg, 0) >> 14, (end - 1) >> 14))
    return out


# ---- rules 4 and 6: the finishing pass -----------------------------------------------------------------------------------------------

def fill_linear(touched):
    """touched: {window: u of the first record that touches it} -> the linear index (rule 4)"""
    if not touched:
        return []
    n = max(touched) + 1
    lin, last = [], touched[min(touched)]
    for w in range(n):
        last = touched.get(w, last)
        lin.append(last)
    return lin


def merge_bins(bins, log=None):
    """bins: {bin: [[u, v]]} of one reference, chunks in file order -> the same after rule 6; log gets (bin, what) with what one of
    "merged", "no_parent", "wide" per bin of levels 5 .. 1 looked at on its own level, and ("join" | "apart", bin) per chunk pair"""
    bins = {b: [list(c) for c in cs] for b, cs in bins.items()}
    for level in (5, 4, 3, 2, 1):
        for b in sorted(bins):
            if bin_level(b) != level:
                continue
            cs = sorted(bins[b])
            bins[b] = cs
            parent = (b - 1) >> 3
            wide = (cs[-1][1] >> 16) - (cs[0][0] >> 16) >= 65536
            what = "no_parent" if parent not in bins else "wide" if wide else "merged"
            if what == "merged":
                bins[parent].extend(cs)
                del bins[b]
            if log is not None:
                log.append((b, what))
    for b, cs in bins.items():
        cs.sort()
        out = [cs[0]]
        for c in cs[1:]:
            join = c[0] >> 16 <= out[-1][1] >> 16
            if join:
                out[-1][1] = max(out[-1][1], c[1])
            else:
                out.append(c)
            if log is not None:
                log.append((b, "join" if join else "apart"))
        bins[b] = out
    return bins


def build(body, rec_off, data_off, comp_off, file_off, n_ref, log=None):
    """-> the parsed form of the index: {"n_ref", "refs": [{"bins": {bin: [[u, v]]}, "linear": [..], "meta": None | [[u, v], [mapped,
    unmapped]]}], "n_no_coor"}"""
    check_arguments(len(body), rec_off, data_off, comp_off, n_ref)
    recs = record_pass(body, rec_off, data_off, comp_off, file_off, n_ref)
    raw = [{} for _ in range(n_ref)]
    touched = [{} for _ in range(n_ref)]
    meta = [None] * n_ref
    n_no_coor, prev = 0, None
    for ref_id, b, u, v, mapped, w0, w1 in recs:
        if ref_id < 0:
            n_no_coor += 1
            prev = None
            continue
        if prev == (ref_id, b):
            raw[ref_id][b][-1][1] = v
        else:
            raw[ref_id].setdefault(b, []).append([u, v])
        prev = (ref_id, b)
        if meta[ref_id] is None:
            meta[ref_id] = [[u, v], [0, 0]]
        meta[ref_id][0][1] = v
        meta[ref_id][1][0 if mapped else 1] += 1
        if mapped:
            for w in range(w0, w1 + 1):
                touched[ref_id].setdefault(w, u)
    refs = []
    for t in range(n_ref):
        ref_log = [] if log is not None else None
        refs.append({"bins": merge_bins(raw[t], ref_log), "linear": fill_linear(touched[t]), "meta": meta[t]})
        if log is not None:
            log.extend((t,) + e for e in ref_log)
            log.extend((t, "window", w in touched[t], w < min(touched[t])) for w in range(len(refs[-1]["linear"])))
    return {"n_ref": n_ref, "refs": refs, "n_no_coor": n_no_coor}


def build_from_file(bam, log=None):
    """the index of a whole BGZF-compressed BAM -> (parsed index, inflated bytes, rec_off, data_off, comp_off, references)"""
    data, data_off, comp_off = file_tables(bam)
    first, refs = parse_header(data)
    rec_off = record_chain(data, first)
    assert rec_off[-1] == len(data)
    return build(data, rec_off, data_off, comp_off, 0, len(refs), log), data, rec_off, data_off, comp_off, refs


# ---- the file (rule 7) ---------------------------------------------------------------------------------------------------------------

def parse_bai(bai):
    assert bai[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", bai, 4)
    o, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", bai, o)
        o += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, o)
            vals = struct.unpack_from("<%dQ" % (2 * n_chunk), bai, o + 8)
            o += 8 + 16 * n_chunk
            chunks = [[vals[2 * i], vals[2 * i + 1]] for i in range(n_chunk)]
            assert b not in bins and (b != META_BIN or meta is None)
            if b == META_BIN:
                assert n_chunk == 2
                meta = chunks
            else:
                bins[b] = chunks
        n_intv, = struct.unpack_from("<i", bai, o)
        linear = list(struct.unpack_from("<%dQ" % n_intv, bai, o + 4))
        o += 4 + 8 * n_intv
        refs.append({"bins": bins, "linear": linear, "meta": meta})
    n_no_coor = 0
    if o + 8 <= len(bai):
        n_no_coor, = struct.unpack_from("<Q", bai, o)
        o += 8
    assert o == len(bai)
    return {"n_ref": n_ref, "refs": refs, "n_no_coor": n_no_coor}


def to_bytes(idx):
    out = [b"BAI\1", struct.pack("<i", idx["n_ref"])]
    for r in idx["refs"]:
        out.append(struct.pack("<i", len(r["bins"]) + (r["meta"] is not None)))
        for b in sorted(r["bins"]):
            out.append(struct.pack("<Ii", b, len(r["bins"][b])) + b"".join(struct.pack("<QQ", *c) for c in r["bins"][b]))
        if r["meta"] is not None:
            out.append(struct.pack("<Ii", META_BIN, 2) + b"".join(struct.pack("<QQ", *c) for c in r["meta"]))
        out.append(struct.pack("<i", len(r["linear"])) + struct.pack("<%dQ" % len(r["linear"]), *r["linear"]))
    out.append(struct.pack("<Q", idx["n_no_coor"]))
    return b"".join(out)


def as_json(idx):
    """bins keyed by strings, as a JSON file holds them"""
    return {"n_ref": idx["n_ref"], "n_no_coor": idx["n_no_coor"],
            "refs": [{"bins": {str(b): r["bins"][b] for b in sorted(r["bins"])}, "linear": r["linear"], "meta": r["meta"]}
                     for r in idx["refs"]]}


def from_json(j):
    return {"n_ref": j["n_ref"], "n_no_coor": j["n_no_coor"],
            "refs": [{"bins": {int(b): [list(c) for c in cs] for b, cs in r["bins"].items()}, "linear": list(r["linear"]),
                      "meta": None if r["meta"] is None else [list(c) for c in r["meta"]]} for r in j["refs"]]}


# ---- the query -----------------------------------------------------------------------------------------------------------------------

def query(idx, tid, beg, end):
    """lfq_bam_index_query: the chunks of every bin of reg2bins(beg, end) whose end lies above the linear index's value for
    beg >> 14 (0 past n_intv), begun no earlier than that value, sorted, overlapping or touching ones merged"""
    if tid < 0 or tid >= idx["n_ref"] or end <= beg or end <= 0:
        return []
    beg, end = max(beg, 0), min(end, MAX_END)
    if beg >= end:
        return []
    r = idx["refs"][tid]
    w = beg >> 14
    min_off = r["linear"][w] if w < len(r["linear"]) else 0
    cs = sorted([max(c[0], min_off), c[1]] for b in reg2bins(beg, end) for c in r["bins"].get(b, ()) if c[1] > min_off)
    out = []
    for c in cs:
        if out and c[0] <= out[-1][1]:
            out[-1][1] = max(out[-1][1], c[1])
        else:
            out.append(c)
    return out


def overlapping(body, rec_off, tid, beg, end):
    """brute force: the mapped records of reference tid with pos < end and end position > beg (a placed unmapped read is in its
    bin but not in the linear index: no query promises it)"""
    out = []
    for j in range(len(rec_off) - 1):
        ref_id, b, e, mapped = record_span(body, rec_off[j])
        if ref_id == tid and mapped and b < end and e > beg:
            out.append(j)
    return out


def reached(chunks, us):
    """the records whose first byte's virtual offset lies in one of the chunks"""
    return [j for j, u in enumerate(us) if any(c[0] <= u < c[1] for c in chunks)]
