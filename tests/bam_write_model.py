"""A restatement, byte by byte, of what `lofreq viterbi`, `lofreq alnqual` and `lofreq indelqual` do to the bytes of a BAM record
(bam_aux_get / bam_aux_del / bam_aux_append, replace_cigar), for the tests of lfq_readset_encode_bam.

rewrite(recs, src, what, ...)   the records dict lfq_readset_encode_bam has to return, in the layout of tests/bam_records.py::encode
edge_cases()                    the edge table of tests/test_gpu_bam_write.py: rows that sit on the constants of the copy pass
tests/test_bam_write_model.py holds rewrite to the 2.1.4 binary (tests/golden/bam_write.json).  No test in here."""
import struct

import numpy as np

import bam_records as br

PUT_ALIGNMENT, DROP_ALN_TAGS, PUT_LB, PUT_IDAQ, KEEP_EXISTING, PUT_INDELQUAL = 1, 2, 4, 8, 16, 32
UNIFORM, DINDEL = 1, 2                                      # LFQ_IDQ_UNIFORM, LFQ_IDQ_DINDEL
# the `what` of the reference's commands
VITERBI, VITERBI_K = PUT_ALIGNMENT | DROP_ALN_TAGS, PUT_ALIGNMENT
ALNQUAL_R, ALNQUAL, ALNQUAL_R_NO_BAQ, ALNQUAL_R_NO_IDAQ = PUT_LB | PUT_IDAQ, PUT_LB | PUT_IDAQ | KEEP_EXISTING, PUT_IDAQ, PUT_LB
INDELQUAL = PUT_INDELQUAL
CHAIN = VITERBI | ALNQUAL_R | INDELQUAL


def aux_fields(aux):
    """[(start, end, tag, type letter)] of the fields of an aux block; ValueError for a malformed one"""
    out, p = [], 0
    while p < len(aux):
        if len(aux) - p < 3:
            raise ValueError("header cut")
        tag, typ = bytes(aux[p:p + 2]), chr(aux[p + 2])
        q = p + 3
        if typ in br.FIXED:
            size = br.FIXED[typ]
        elif typ in "ZH":
            e = aux.find(b"\0", q)
            if e < 0:
                raise ValueError("no NUL")
            size = e - q + 1
        elif typ == "B":
            if len(aux) - q < 5 or chr(aux[q]) not in br.FIXED or chr(aux[q]) == "A":
                raise ValueError("B header")
            size = 5 + br.FIXED[chr(aux[q])] * struct.unpack("<I", aux[q + 1:q + 5])[0]
        else:
            raise ValueError("type %r" % typ)
        if q + size > len(aux):
            raise ValueError("value cut")
        out.append((p, q + size, tag, typ))
        p = q + size
    return out


def _first(fields, tag, gone):
    """bam_aux_get: the index of the first field with `tag` among those not yet deleted, whatever its type, or None"""
    for i, f in enumerate(fields):
        if i not in gone and f[2] == tag:
            return i
    return None


def rewrite_one(rec, l_qname, n_cigar, l_qseq, flag, what, new_cigar, lb, ai, ad, tag_flag, bi, bd, idq_mode):
    """one record (bytes from read_name on) -> its new bytes.  new_cigar: uint32 words of the read set's CIGAR; lb / ai / ad / bi /
    bd: the l_qseq tag bytes of the read (or None where `what` has no use for them); tag_flag: bit 0 / 1 = the read got ai / ad"""
    rec = bytes(rec)
    l = int(l_qseq)
    a0 = int(l_qname) + 4 * int(n_cigar)
    a1 = a0 + (l + 1) // 2 + l
    qname, cigar, seqqual, aux = rec[:int(l_qname)], rec[int(l_qname):a0], rec[a0:a1], rec[a1:]
    fields = aux_fields(aux)
    new_cigar = np.asarray(new_cigar, "<u4")
    gone, tail = set(), []
    if what & PUT_ALIGNMENT:                                # replace_cigar, lofreq_viterbi.c:340
        cigar = new_cigar.tobytes()
    if what & DROP_ALN_TAGS:                                # lofreq_viterbi.c:119-146: before the flag is looked at
        for tag in (b"NM", b"MC", b"MD", b"AS"):
            i = _first(fields, tag, gone)
            if i is not None:
                gone.add(i)
    if what & (PUT_LB | PUT_IDAQ) and not (flag & 4) and l > 0:         # bam_md_ext.c:291
        present = {}
        for tag, selected in ((b"lb", what & PUT_LB), (b"ai", what & PUT_IDAQ), (b"ad", what & PUT_IDAQ)):
            i = _first(fields, tag, gone)
            present[tag] = i is not None
            if i is not None and fields[i][3] == "Z" and selected and not what & KEEP_EXISTING:       # :297-314
                gone.add(i)
                present[tag] = False
        ops = new_cigar & 0xf
        has_ins, has_del = bool((ops == 1).any()), bool((ops == 2).any())
        skip = (not what & PUT_LB or present[b"lb"]) and (not has_del or present[b"ad"]) and (not has_ins or present[b"ai"])
        if not skip:                                        # :352-366
            if what & PUT_LB and not present[b"lb"]:        # :409, :472
                tail.append((b"lb", lb))
            if what & PUT_IDAQ and (has_ins or has_del):    # :478, :241-246 -- whatever present[] says
                if tag_flag & 1:
                    tail.append((b"ai", ai))
                if tag_flag & 2:
                    tail.append((b"ad", ad))
    if what & PUT_INDELQUAL and (idq_mode == UNIFORM or not (flag & 0x704)):    # lofreq_indelqual.c:69-104, :143-148
        for tag, val in ((b"BI", bi), (b"BD", bd)):
            i = _first(fields, tag, gone)
            if i is not None:
                gone.add(i)
            tail.append((tag, val))
    out = qname + cigar + seqqual + b"".join(aux[f[0]:f[1]] for i, f in enumerate(fields) if i not in gone)
    for tag, val in tail:
        val = bytes(val) if isinstance(val, (bytes, bytearray)) else np.asarray(val, np.uint8).tobytes()
        assert len(val) == l, (tag, len(val), l)
        out += tag + b"Z" + val + b"\0"
    return out


def rewrite(recs, src, what, new_pos, new_cigars, lb, ai, ad, tag_flags, bi, bd, idq_mode):
    """recs: the original records (tests/bam_records.py::encode layout); src[j]: the record of read j of the read set (None: the
    identity); new_pos [n], new_cigars (list of uint32 arrays): the read set's, in ITS read order; lb, ai, ad, bi, bd: the read
    set's per-base tag bytes in its seq_off layout (None where `what` does not need them); tag_flags [n]: bit 0 / 1 = read j got
    ai / ad (ReadSet.fetch_tags); idq_mode: UNIFORM / DINDEL.  -> the records dict, records in the read set's order"""
    n = len(recs["pos"])
    src = np.arange(n, dtype=np.int64) if src is None else np.asarray(src, np.int64)
    data = bytes(np.asarray(recs["data"], np.uint8))
    so = np.concatenate([[0], np.cumsum(np.asarray(recs["l_qseq"], np.int64)[src])]).astype(np.int64)
    parts, off, pos, nc = [], [0], [], []
    part = lambda a, j: None if a is None else np.asarray(a, np.uint8)[so[j]:so[j + 1]]
    for j in range(n):
        s = int(src[j])
        rec = data[int(recs["data_off"][s]):int(recs["data_off"][s + 1])]
        new = rewrite_one(rec, recs["l_qname"][s], recs["n_cigar"][s], recs["l_qseq"][s], int(recs["flag"][s]), what,
                          new_cigars[j], part(lb, j), part(ai, j), part(ad, j), 0 if tag_flags is None else int(tag_flags[j]),
                          part(bi, j), part(bd, j), idq_mode)
        parts.append(new)
        off.append(off[-1] + len(new))
        pos.append(int(new_pos[j]) if what & PUT_ALIGNMENT else int(recs["pos"][s]))
        nc.append(len(new_cigars[j]) if what & PUT_ALIGNMENT else int(recs["n_cigar"][s]))
    out = {"data": np.frombuffer(b"".join(parts), np.uint8).copy() if off[-1] else np.zeros(0, np.uint8),
           "data_off": np.asarray(off, np.int64), "pos": np.asarray(pos, np.int32).reshape(n),
           "n_cigar": np.asarray(nc, np.uint32).reshape(n), "src": src}
    for k in ("flag", "mapq", "l_qname", "l_qseq"):
        out[k] = np.asarray(recs[k])[src]
    if "ref" in recs:
        out["ref"] = recs["ref"]
    return out


def record_cigars(recs):
    """the CIGAR words of every record, as the list rewrite takes"""
    data = np.asarray(recs["data"], np.uint8)
    out = []
    for r in range(len(recs["pos"])):
        p = int(recs["data_off"][r]) + int(recs["l_qname"][r])
        out.append(np.frombuffer(data[p:p + 4 * int(recs["n_cigar"][r])].tobytes(), "<u4").astype(np.uint32))
    return out


# ---- the edge table -----------------------------------------------------------------------------------------------------------------
# A row: reads (dicts for bam_records.encode; "aux_raw" = the aux block), keyword arguments of encode, and
#   what       LFQ_BAM_* bits
#   idq        None / UNIFORM / DINDEL: lfq_readset_indelqual runs in that mode
#   baq        lfq_readset_baq(want_idaq = 1) runs (reads of such rows are mapped and have an M operation)
#   reverse    the read set holds the reads in reversed order, src = n-1 .. 0
#   set_cigar  a function read index -> CIGAR: the READ SET is made of records with these CIGARs (the same query length) instead,
#              which is what PUT_ALIGNMENT then writes into the original records

REF = ("ACGTTGCAAGGCTTAACCGGATCGATTACAGGCATCGAGCTA" * 12).encode()


def mk(l, seed=0, aux=b"", flag=0, cigar=None, name="r"):
    r = br.mk(l, seed, tags=None, name=name)
    r["aux_raw"] = bytes(aux)
    r["flag_other"] = flag
    if cigar is not None:
        r["cigar"] = cigar
    return r


def indel_cigar(l, kind):
    """a CIGAR of query length l >= 8 with an insertion ("i"), a deletion ("d"), both ("b") or neither ("m")"""
    if l < 8 or kind == "m":
        return [("M", l)]
    if kind == "i":
        return [("M", 3), ("I", 2), ("M", l - 5)]
    if kind == "d":
        return [("M", 4), ("D", 3), ("M", l - 4)]
    return [("M", 2), ("I", 1), ("M", 2), ("D", 2), ("M", l - 5)]


def z(tag, n, byte=65):
    return br.aux_field(tag, "Z", bytes([byte]) * n)


def edge_cases():
    chunks = br.source_constant("LFQ_BAM_COPY_CHUNKS")
    plan_reads = br.source_constant("LFQ_BAM_PLAN_READS")
    tile = 16 * chunks
    every = b"".join(br.one_of_every_type())
    nm, md, as_, mc = br.aux_field("NM", "i", b"\1\0\0\0"), z("MD", 5), br.aux_field("AS", "C", b"\x20"), z("MC", 3)
    cases = {}
    row = lambda reads, what, kw=None, idq=None, baq=False, reverse=False, set_cigar=None: dict(
        reads=reads, kw=kw or {}, what=what, idq=idq, baq=baq, reverse=reverse, set_cigar=set_cigar)
    kinds = "midb"
    for l in (1, 2, 15, 16, 17, 31, 33):
        reads = [mk(l, s, aux=(b"", nm + z("lb", l), z("BI", l) + md, every)[s % 4], cigar=indel_cigar(l, kinds[s % 4])) for s in range(6)]
        cases["l_qseq_%d" % l] = row(reads, CHAIN & ~PUT_ALIGNMENT, idq=DINDEL, baq=True)
    for o in range(4):
        reads = [mk(9 + s, s, aux=(nm, b"", md + every)[s % 3]) for s in range(9)]
        cases["first_record_at_offset_%d" % o] = row(reads, VITERBI | INDELQUAL, kw={"first_offset": o}, idq=UNIFORM)
    # qname lengths 1 .. 16 with a fixed rest: the output records start at every offset mod 16
    reads = [mk(12, s, aux=nm + z("XX", s % 5)) for s in range(48)]
    cases["output_records_at_every_offset_mod_16"] = row(reads, DROP_ALN_TAGS | INDELQUAL, kw={"qname_len": [1 + s % 16 for s in range(48)]},
                                                          idq=UNIFORM)
    x1, x2 = br.aux_field("XA", "c", b"\7"), z("XB", 21, 66)
    for name, aux in (("deletion_at_the_front", nm + x1 + x2), ("deletion_in_the_middle", x1 + nm + x2),
                      ("deletion_at_the_end", x1 + x2 + nm), ("two_adjacent_deletions", x1 + nm + md + x2),
                      ("two_separate_deletions", nm + x1 + md + x2 + as_), ("all_aux_deleted", nm + mc + md + as_),
                      ("no_aux_at_all", b""), ("second_field_of_a_tag_stays", nm + x1 + nm + md + md),
                      ("nine_deletions", nm + x1 + mc + x1 + md + x1 + as_ + x1 + z("lb", 20) + x1 + z("ai", 20) + x1 + z("ad", 20)
                       + x1 + z("BI", 20) + x1 + z("BD", 20) + x1)):
        reads = [mk(20, 1, aux=aux, cigar=indel_cigar(20, "b")), mk(7, 2, aux=x1), mk(20, 3, aux=aux, cigar=indel_cigar(20, "m"))]
        cases[name] = row(reads, CHAIN & ~PUT_ALIGNMENT, idq=DINDEL, baq=True)
    # appended fields across a 16-byte and a tile boundary: records of 8 + 4 + (l + 1) / 2 + l bytes and two fields of l + 4 each;
    # every l from 20 to 51 moves the heads, payloads and NULs over all chunk offsets, and enough of them pass the first tile end
    reads = [mk(20 + s % 32, s) for s in range(2 * tile // 60 + 40)]
    cases["appended_fields_straddle_chunks_and_tiles"] = row(reads, INDELQUAL, kw={"qname_len": 8}, idq=UNIFORM)
    big = z("XL", tile + 300, 67)
    cases["record_longer_than_a_tile"] = row([mk(9, 1, aux=nm), mk(30, 2, aux=nm + big + md), mk(11, 3, aux=big + big + nm), mk(5, 4)],
                                             DROP_ALN_TAGS | INDELQUAL, idq=UNIFORM)
    many = lambda n: [mk((1, 2, 15, 16, 17, 31, 33, 60)[i % 8], i, aux=(b"", nm, z("BD", 4) + md, every + as_)[i % 4]) for i in range(n)]
    for n in (1, 63, 64, 65, plan_reads + 1):
        cases["%d_reads" % n] = row(many(n), VITERBI | INDELQUAL, idq=DINDEL)
    grown = lambda i: indel_cigar(24, "b")
    cases["n_cigar_grows"] = row([mk(24, s, aux=nm + x2) for s in range(5)], VITERBI, set_cigar=grown)
    cases["n_cigar_shrinks"] = row([mk(24, s, aux=x2 + nm, cigar=indel_cigar(24, "b")) for s in range(5)], VITERBI_K,
                                   set_cigar=lambda i: [("M", 24)])
    cases["reversed_src"] = row(many(37), CHAIN & ~PUT_ALIGNMENT, idq=DINDEL, baq=True, reverse=True)
    flags = [0, 4, 256, 512, 1024, 16, 4 | 1024]
    tagged = z("lb", 18) + br.aux_field("ai", "A", b"x") + z("BI", 18) + nm
    for name, what, idq in (("viterbi", VITERBI, None), ("viterbi_k", VITERBI_K, None), ("alnqual_r", ALNQUAL_R, None),
                            ("alnqual", ALNQUAL, None), ("alnqual_r_no_baq", ALNQUAL_R_NO_BAQ, None),
                            ("alnqual_r_no_idaq", ALNQUAL_R_NO_IDAQ, None), ("indelqual_uniform", INDELQUAL, UNIFORM),
                            ("indelqual_dindel", INDELQUAL, DINDEL), ("chain", CHAIN, DINDEL), ("chain_uniform", CHAIN, UNIFORM)):
        reads = [mk(18, s, aux=(tagged, b"", z("ad", 18) + z("ai", 18))[s % 3], flag=flags[s % 7],
                    cigar=indel_cigar(18, kinds[(s // 3) % 4] if not flags[s % 7] & 4 else "m")) for s in range(21)]
        cases["what_" + name] = row(reads, what, idq=idq, baq=bool(what & (PUT_LB | PUT_IDAQ)))
    return cases
