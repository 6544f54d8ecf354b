"""The stored-tag decode (lfq_readset_create_from_bam_tags) and the merge rule of lfq_readset_baq_fill, restated in Python from
bam_prob_realn_core_ext (bam_md_ext.c:291-366, :409, :472, :241-246) for the tests that hold both against the 2.1.4 binary
(test_tag_reuse_model.py) and the device code against this (test_gpu_tag_reuse.py).

first_fields(aux)          the first lb / ai / ad field of an aux block: {tag: (type letter, string or None)}
stored_tags(recs, tags)    what the decode keeps of the records of bam_records.encode: per-base arrays and per-read bits;
                           Unusable where the first field of a selected tag is no Z string of at least l_qseq bytes
need_hmm / merge_read      the rule for one read
merge(...)                 the rule over the arrays of a batch: what lfq_readset_fetch_tags must give after the fill
No test in here."""
import struct

import numpy as np

import bam_records as br

TAGS = (b"lb", b"ai", b"ad")
READ_LB, READ_IDAQ = 1, 2


class Unusable(ValueError):
    """the first field of a selected tag cannot be used: LFQ_ERR_INVALID from the decode"""


def first_fields(aux):
    """{tag: (type, z)} of the FIRST lb / ai / ad field of the aux block (bam_aux_get): z = the string of a Z / H field, else None"""
    out, p = {}, 0
    aux = bytes(aux)
    while p + 3 <= len(aux):
        t, typ = aux[p:p + 2], chr(aux[p + 2])
        p += 3
        if typ in br.FIXED:
            size, z = br.FIXED[typ], None
        elif typ in "ZH":
            e = aux.index(b"\0", p)
            size, z = e - p + 1, aux[p:e]
        elif typ == "B":
            size, z = 5 + br.FIXED[chr(aux[p])] * struct.unpack("<I", aux[p + 1:p + 5])[0], None
        else:
            raise ValueError("aux type %r" % typ)
        if t in TAGS and t not in out:
            out[t] = (typ, z)
        p += size
    return out


def record_aux(recs, r):
    o0, o1 = int(recs["data_off"][r]), int(recs["data_off"][r + 1])
    l, nc = int(recs["l_qseq"][r]), int(recs["n_cigar"][r])
    p = o0 + int(recs["l_qname"][r]) + 4 * nc + (l + 1) // 2 + l
    return bytes(np.asarray(recs["data"], np.uint8)[p:o1])


def stored_tags(recs, read_tags=READ_LB | READ_IDAQ):
    """-> {"lb", "ai", "ad": uint8 per base ('!' for a read without the tag), "flags": uint8 per read, bit 0 / 1 / 2}"""
    n = len(recs["pos"])
    per = {t: [] for t in TAGS}
    flags = np.zeros(n, np.uint8)
    selected = [t for bit, t in ((READ_LB, b"lb"), (READ_IDAQ, b"ai"), (READ_IDAQ, b"ad")) if read_tags & bit]
    for r in range(n):
        l = int(recs["l_qseq"][r])
        ff = first_fields(record_aux(recs, r))
        for k, t in enumerate(TAGS):
            if t in selected and t in ff:
                typ, z = ff[t]
                if typ != "Z" or len(z) < l:
                    raise Unusable("read %d: first %s field of type %s, %s bytes for %d bases" % (r, t.decode(), typ, z and len(z), l))
                per[t].append(np.frombuffer(z[:l], np.uint8))
                flags[r] |= 1 << k
            else:
                per[t].append(np.full(l, 33, np.uint8))
    cat = lambda xs: np.concatenate(xs + [np.zeros(0, np.uint8)]).astype(np.uint8)
    return {"lb": cat(per[b"lb"]), "ai": cat(per[b"ai"]), "ad": cat(per[b"ad"]), "flags": flags}


def has_ins_del(cigar):
    """cigar: [(op letter, length)]"""
    return any(op == "I" for op, _ in cigar), any(op == "D" for op, _ in cigar)


def effective_bits(S, want_idaq, redo_baq):
    """the stored bits that count: S_lb is 0 under redo_baq (baq_flag = 2 deletes the tag, :297-302), S_ai / S_ad without
    want_idaq (nothing reads them)"""
    return (S & (0 if redo_baq else 1)) | (S & (6 if want_idaq else 0))


def need_hmm(S, has_ins, has_del, want_idaq):
    """bam_md_ext.c:352-366 on the effective bits; without want_idaq a run for missing ai / ad would write nothing"""
    return not (S & 1) or bool(want_idaq and ((has_del and not (S & 4)) or (has_ins and not (S & 2))))


def merge_read(stored, computed, has_ins, has_del, want_idaq, redo_baq):
    """one read.  stored / computed: {"lb", "ai", "ad"} -> bytes or None (no such field).  -> (result dict of the same form: the
    FIRST field of each tag after the reference's run, need_hmm)"""
    S = sum(1 << k for k, t in enumerate(("lb", "ai", "ad")) if stored.get(t) is not None)
    S = effective_bits(S, want_idaq, redo_baq)
    need = need_hmm(S, has_ins, has_del, want_idaq)
    out = {"lb": stored["lb"] if S & 1 else computed["lb"]}
    for k, t in ((1, "ai"), (2, "ad")):
        if not want_idaq:
            out[t] = None
        elif S & (1 << k):
            out[t] = stored[t]
        else:
            out[t] = computed.get(t) if need else None
    return out, need


def merge(seq_off, cigars, stored, computed, want_idaq, redo_baq):
    """the batch: stored = stored_tags(...), computed = {"lb", "ai", "ad": per base, "flags": per read, bit 0 / 1 = ai / ad} as
    lfq_readset_baq + lfq_readset_fetch_tags give them on the same reads (ai / ad / flags None without want_idaq).
    -> (lb, ai, ad, flags, need) as lfq_readset_fetch_tags must give them after the fill; an absent ai / ad is '~' bytes, flag clear"""
    n = len(cigars)
    lb = computed["lb"].copy()
    ai = computed["ai"].copy() if want_idaq else None
    ad = computed["ad"].copy() if want_idaq else None
    fl = np.zeros(n, np.uint8)
    need = np.zeros(n, bool)
    for r in range(n):
        a, b = int(seq_off[r]), int(seq_off[r + 1])
        hi, hd = has_ins_del(cigars[r])
        sf, cf = int(stored["flags"][r]), int(computed["flags"][r]) if want_idaq else 0
        st = {t: (stored[t][a:b] if sf & (1 << k) else None) for k, t in enumerate(("lb", "ai", "ad"))}
        co = {"lb": computed["lb"][a:b], "ai": computed["ai"][a:b] if cf & 1 else None, "ad": computed["ad"][a:b] if cf & 2 else None}
        out, need[r] = merge_read(st, co, hi, hd, want_idaq, redo_baq)
        lb[a:b] = out["lb"]
        for k, (t, arr) in enumerate((("ai", ai), ("ad", ad))):
            if want_idaq:
                arr[a:b] = out[t] if out[t] is not None else 126
                fl[r] |= (1 << k) if out[t] is not None else 0
    return lb, ai, ad, fl, need


# ---- the fixture tests/golden/tag_reuse.json (tests/make_tagreuse_golden.py) ---------------------------------------------------

BI_BYTE, BD_BYTE = 33 + 45, 33 + 44        # every read of the fixture carries these indel qualities


def fixture_reads(fx, strip=False):
    """the reads of the fixture in the dict form bam_records.encode takes, aux block included: BI, BD, then the foreign lb / ai /
    ad strings (a constant byte, l_qseq + extra bytes long) unless strip.  read = [pos0, flag, mapq, cigar, letters, qual,
    {tag: [byte, extra]}]"""
    import golden_util as gu
    out = []
    for i, (pos0, flag, mapq, cigar, letters, qual, tags) in enumerate(fx["reads"]):
        l = len(letters)
        aux = br.aux_field("BI", "Z", bytes([BI_BYTE]) * l) + br.aux_field("BD", "Z", bytes([BD_BYTE]) * l)
        for t in ("lb", "ai", "ad"):
            if t in tags and not strip:
                aux += br.aux_field(t, "Z", bytes([tags[t][0]]) * (l + tags[t][1]))
        out.append({"name": "q%d" % i, "pos0": pos0, "reverse": bool(flag & 16), "mapq": mapq, "cigar": gu.parse_cigar(cigar),
                    "seq": np.array(["ACGTN".index(c) for c in letters], np.uint8),
                    "qual": np.array([ord(c) - 33 for c in qual], np.uint8), "aux_raw": aux})
    return out


def fixture_records(fx, strip=False):
    reads = fixture_reads(fx, strip)
    return reads, br.encode(reads, ref=fx["genome"].encode(), qname_len=[len(r["name"]) + 1 for r in reads])
