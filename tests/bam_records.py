"""BAM records as they lie in memory (bam1_t.data), for the tests of lfq_readset_create_from_bam and lfq_region_add_record.

encode(reads, ...)      reads in the dict form of tests/golden_reads.py / test_gpu_chain.py::_bam_fields -> the arrays of an
                        lfq_bam_records: one byte buffer (qname | cigar | 4-bit seq | qual | aux per read) and the descriptors
expected_arrays(recs)   a numpy restatement of what the per-base host loop makes of such records: lfq_region_add_read's loop
                        (integration/lofreq_amd_region.c) behind bam_aux_get(b, "BI") / bam_aux_get(b, "BD") -- read from the
                        BYTES of the records, not from the dicts they were encoded from
No test in here."""
import os
import re
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = "MIDNSHP=X"
# 4-bit BAM base "=ACMGRSVTWYHKDBN" -> the library's base code (lofreq_amd_region.c, nt16_int)
NT16_INT = np.array([5, 0, 1, 6, 2, 7, 8, 9, 3, 10, 11, 12, 13, 14, 15, 4], np.uint8)
CODE_TO_NIBBLE = np.argsort(NT16_INT).astype(np.uint8)
FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def source_constant(name, path="lofreq_amd/csrc/lfq_bamrec.hip"):
    return int(re.search(r"#define %s (\d+)" % name, open(os.path.join(ROOT, path)).read()).group(1))


def aux_field(tag, typ, value=b""):
    """one aux field: tag (2 letters), type letter, value -- bytes as they are for the fixed types, the string WITHOUT its NUL
    for Z / H, (subtype letter, count, payload bytes) for B"""
    head = tag.encode() + typ.encode()
    if typ in "ZH":
        return head + bytes(value) + b"\0"
    if typ == "B":
        sub, count, payload = value
        return head + sub.encode() + struct.pack("<I", count) + bytes(payload)
    return head + bytes(value)


def one_of_every_type():
    """a field of every fixed type, a Z, an H, and a B of each subtype incl. count 0 (none of them tagged BI / BD)"""
    out = [aux_field("X" + t, t, bytes(range(1, FIXED[t] + 1))) for t in "AcCsSif"] + [aux_field("XI", "I", b"\1\2\3\4")]
    out += [aux_field("XZ", "Z", b"BI:Z:decoy"), aux_field("XH", "H", b"1AE301"), aux_field("XE", "Z", b"")]
    for k, sub in enumerate("cCsSiIf"):
        out.append(aux_field("Y" + sub, "B", (sub, k % 3, bytes(range(FIXED[sub] * (k % 3))))))
    out.append(aux_field("Y0", "B", ("c", 0, b"")))
    return out


def record_fields(r, qname_len=None, before=(), after=()):
    """-> (l_qname, n_cigar, l_qseq, data bytes) of one read: r["nib"] (raw 4-bit codes) or r["seq"] (base codes 0..15), r["qual"],
    r["cigar"], optional r["bi"] / r["bd"] (tag bytes per base); r["aux_raw"] (bytes) replaces the aux block altogether"""
    nib = np.asarray(r["nib"], np.uint8) if "nib" in r else CODE_TO_NIBBLE[np.asarray(r["seq"], np.uint8)]
    l = len(nib)
    if l & 1:
        nib = np.append(nib, 0).astype(np.uint8)
    seq4 = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes()
    qual = np.asarray(r["qual"], np.uint8)
    assert len(qual) == l
    cig = np.asarray([(ln << 4) | OPS.index(o) for o, ln in r["cigar"]], "<u4").tobytes()
    if qname_len is None:
        qname_len = (len(r.get("name", "r")) + 1 + 3) // 4 * 4       # htslib pads l_qname to a multiple of 4
    name = r.get("name", "r").encode()[: qname_len - 1]
    qname = name + b"\0" * (qname_len - len(name))
    if "aux_raw" in r:
        aux = bytes(r["aux_raw"])
    else:
        aux = b"".join(before)
        for tag in ("bi", "bd"):
            if r.get(tag) is not None:
                aux += aux_field(tag.upper(), "Z", np.asarray(r[tag], np.uint8).tobytes())
        aux += b"".join(after)
    return qname_len, len(r["cigar"]), l, qname + cig + seq4 + qual.tobytes() + aux


def encode(reads, ref=b"", qname_len=None, before=(), after=(), first_offset=0):
    """-> dict with the arrays of an lfq_bam_records (+ "ref").  qname_len: one length for every read, a list, or None (htslib's
    padding); before / after: aux fields around BI / BD; first_offset: bytes of padding in front of the first record"""
    n = len(reads)
    parts, off = [b"\xa5" * first_offset], [first_offset]
    lq, nc, ls = [], [], []
    for i, r in enumerate(reads):
        q = qname_len[i] if isinstance(qname_len, (list, tuple)) else qname_len
        a, b, c, data = record_fields(r, q, before, after)
        lq.append(a); nc.append(b); ls.append(c)
        parts.append(data)
        off.append(off[-1] + len(data))
    return {"data": np.frombuffer(b"".join(parts) + b"", np.uint8).copy() if off[-1] else np.zeros(0, np.uint8),
            "data_off": np.asarray(off, np.int64),
            "pos": np.asarray([r["pos0"] for r in reads], np.int32).reshape(n),
            "flag": np.asarray([(16 if r.get("reverse") else 0) | (r.get("flag_other", 0) & ~16) for r in reads], np.uint16).reshape(n),
            "mapq": np.asarray([r.get("mapq", 60) for r in reads], np.uint8).reshape(n),
            "l_qname": np.asarray(lq, np.uint16).reshape(n), "n_cigar": np.asarray(nc, np.uint32).reshape(n),
            "l_qseq": np.asarray(ls, np.int32).reshape(n), "ref": bytes(ref)}


def _aux_get(aux, tag):
    """bam_aux_get + bam_aux2Z: the string of the FIRST field with `tag` if that field is of type Z, else None"""
    p = 0
    while p + 3 <= len(aux):
        t, typ = aux[p:p + 2], chr(aux[p + 2])
        p += 3
        if typ in FIXED:
            size, z = FIXED[typ], None
        elif typ in "ZH":
            e = aux.index(b"\0", p)
            size, z = e - p + 1, aux[p:e]
        elif typ == "B":
            size, z = 5 + FIXED[chr(aux[p])] * struct.unpack("<I", aux[p + 1:p + 5])[0], None
        else:
            raise ValueError("aux type %r" % typ)
        if t == tag:
            return z if typ == "Z" else None
        p += size
    return None


def expected_arrays(recs):
    """the arrays lfq_region_add_read's loop builds from these records (and region_start hands to lfq_readset_create): seq, qual,
    bi, bd per base (bi / bd '!' where the read has no such tag), flags per read, any_bi / any_bd, and the per-read arrays"""
    data = bytes(np.asarray(recs["data"], np.uint8))
    n = len(recs["pos"])
    seq, qual, bi, bd, cig = [], [], [], [], []
    flags = np.zeros(n, np.uint8)
    for r in range(n):
        o0, o1 = int(recs["data_off"][r]), int(recs["data_off"][r + 1])
        l, nc = int(recs["l_qseq"][r]), int(recs["n_cigar"][r])
        p = o0 + int(recs["l_qname"][r])
        cig.append(np.frombuffer(data[p:p + 4 * nc], "<u4").astype(np.uint32))
        p += 4 * nc
        packed = np.frombuffer(data[p:p + (l + 1) // 2], np.uint8)
        i = np.arange(l)
        seq.append(NT16_INT[(packed[i >> 1] >> ((~i & 1) << 2)) & 0xf])            # bam_seqi
        p += (l + 1) // 2
        qual.append(np.frombuffer(data[p:p + l], np.uint8))
        aux = data[p + l:o1]
        for bit, (tag, dst) in enumerate(((b"BI", bi), (b"BD", bd))):
            z = _aux_get(aux, tag)
            if z is not None and len(z) >= l:
                dst.append(np.frombuffer(z[:l], np.uint8))
                flags[r] |= 1 << bit
            else:
                dst.append(np.full(l, 33, np.uint8))
    cat = lambda xs, dt: np.concatenate(xs + [np.zeros(0, dt)]).astype(dt)
    return {"seq": cat(seq, np.uint8), "qual": cat(qual, np.uint8), "bi": cat(bi, np.uint8), "bd": cat(bd, np.uint8),
            "flags": flags, "any_bi": bool((flags & 1).any()), "any_bd": bool((flags & 2).any()),
            "pos": np.asarray(recs["pos"], np.int32), "mapq": np.asarray(recs["mapq"], np.uint8),
            "rev": ((np.asarray(recs["flag"], np.uint16) >> 4) & 1).astype(np.uint8),
            "cig": cat(cig, np.uint32), "cig_off": np.concatenate([[0], np.cumsum(recs["n_cigar"])]).astype(np.int64),
            "seq_off": np.concatenate([[0], np.cumsum(recs["l_qseq"])]).astype(np.int64)}


# ---- the edge table ---------------------------------------------------------------------------------------------------------

def mk(l, seed=0, pos0=None, tags="both", name="r"):
    """a read of l bases, all M; tags: which of BI / BD it carries ("both", "bi", "bd", None)"""
    rng = np.random.default_rng(1000 * l + seed)
    r = {"pos0": int(seed % 50) if pos0 is None else pos0, "cigar": [("M", l)], "seq": rng.integers(0, 5, l).astype(np.uint8),
         "qual": rng.integers(2, 42, l).astype(np.uint8), "mapq": int(20 + seed % 40), "reverse": bool(seed & 1), "name": name}
    if tags in ("both", "bi"):
        r["bi"] = (33 + rng.integers(0, 60, l)).astype(np.uint8)
    if tags in ("both", "bd"):
        r["bd"] = (33 + rng.integers(0, 60, l)).astype(np.uint8)
    return r


def _bi_aux(l, dl=0, typ="Z", seed=7):
    return aux_field("BI", typ, (33 + (np.arange(l + dl) * seed) % 60).astype(np.uint8).tobytes() if typ != "A" else b"I")


def edge_cases():
    """name -> (reads, keyword arguments of encode)"""
    chunks = source_constant("LFQ_BAM_BASE_CHUNKS")
    aux_reads = source_constant("LFQ_BAM_AUX_READS")
    many = lambda n: [mk((1, 2, 15, 16, 17, 31, 33, 150)[i % 8], seed=i, tags=("both", "bi", "bd", None)[i % 4]) for i in range(n)]
    cases = {}
    for l in (1, 2, 15, 16, 17, 31, 33):
        cases["l_qseq_%d" % l] = ([mk(l, 1), mk(l, 2, tags="bi"), mk(l, 3, tags=None), mk(l, 4, tags="bd")], {})
    r = mk(16, 5)
    r.pop("seq")
    r["nib"] = np.arange(16, dtype=np.uint8)
    odd = mk(17, 6)
    odd.pop("seq")
    odd["nib"] = np.arange(16, -1, -1, dtype=np.uint8) % 16
    cases["all_16_nibble_codes"] = ([mk(1, 9), r, odd], {})
    q = mk(33, 7)
    q["qual"][:] = 0xff
    cases["quality_0xff"] = ([q, mk(5, 8)], {})
    for o in range(4):
        cases["first_record_at_offset_%d" % o] = (many(9), {"first_offset": o})
    cases["qnames_leave_the_cigar_unaligned"] = (many(12), {"qname_len": [1 + (i * 7) % 11 for i in range(12)]})
    cases["no_aux_at_all"] = ([mk(20, i, tags=None) for i in range(5)], {})
    cases["bi_only"] = ([mk(20, i, tags="bi") for i in range(5)], {})
    cases["bd_only"] = ([mk(20, i, tags="bd") for i in range(5)], {})
    cases["bi_and_bd"] = ([mk(20, i) for i in range(5)], {})
    for what, dl in (("one_shorter", -1), ("equal", 0), ("longer", 3)):
        r = mk(19, 11, tags=None)
        r["aux_raw"] = _bi_aux(19, dl) + aux_field("BD", "Z", bytes([40] * 19))
        cases["bi_%s_than_l_qseq" % what] = ([mk(7, 1), r, mk(7, 2)], {})
    for typ in "HA":
        r = mk(6, 12, tags=None)
        r["aux_raw"] = _bi_aux(6, 0, typ) + aux_field("BD", "Z", bytes([50] * 6)) + _bi_aux(6, 0, "Z")
        cases["bi_of_type_%s_is_ignored" % typ] = ([r, mk(6, 3)], {})
    r = mk(10, 13, tags=None)
    r["aux_raw"] = _bi_aux(10, 0, seed=3) + _bi_aux(10, 0, seed=5)
    cases["two_bi_fields_first_wins"] = ([r], {})
    r = mk(10, 14, tags=None)
    r["aux_raw"] = _bi_aux(10, -2) + _bi_aux(10, 0, seed=5)            # the first one is too short: the read has no BI
    cases["two_bi_fields_first_too_short"] = ([r, mk(3, 1)], {})
    cases["tags_behind_every_type"] = (many(6), {"before": one_of_every_type()})
    cases["tags_in_front_of_every_type"] = (many(6), {"after": one_of_every_type()})
    cases["bd_nul_is_the_last_byte"] = ([mk(9, 1, tags=None), mk(12, 2, tags="bd")], {})
    for n in (1, 63, 64, 65, chunks + 1, aux_reads + 1):
        cases["%d_reads" % n] = (many(n), {})
    cases["chunks_plus_one_short_reads"] = ([mk(1 + i % 3, i, tags=("bi", None)[i % 2]) for i in range(16 * chunks // 2 + 40)], {})
    cases["reads_longer_than_a_workgroups_tile"] = ([mk(7, 1), mk(16 * chunks + 5, 2, tags="bd"), mk(3 * 16 * chunks, 3), mk(9, 4, tags=None)], {})
    cases["many_tiles"] = (many(3000), {"first_offset": 1})
    cases["only_the_last_read_has_bi"] = ([mk(30, i, tags=None) for i in range(70)] + [mk(30, 99, tags="bi")], {})
    return cases


def malformed_cases():
    """name -> aux bytes of a record whose aux block is malformed"""
    return {"unknown_type": aux_field("XA", "C", b"\1") + b"XQq\1\2",
            "unknown_b_subtype": b"XBBd" + struct.pack("<I", 1) + bytes(8),
            "b_count_past_the_record": b"XBBs" + struct.pack("<I", 1000) + bytes(6),
            "z_without_nul": aux_field("XI", "i", b"\1\0\0\0") + b"XZZabcdef",
            "h_without_nul": b"XHH1A2B",
            "header_cut_by_the_record_end": aux_field("XA", "A", b"x") + b"XY",
            "value_cut_by_the_record_end": b"XIi\1\2"}
