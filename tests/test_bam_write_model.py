"""CPU tests of lfq_readset_encode_bam's rules and ABI: tests/bam_write_model.py::rewrite reproduces, byte for byte, what the 2.1.4
binary's `lofreq viterbi`, `lofreq alnqual` and `lofreq indelqual` made of hand-made records (tests/golden/bam_write.json, from
tests/make_bamwrite_golden.py) -- the new positions, CIGARs and tag strings are taken from the binary's output, so that this is
about the byte rules and not about the HMM --, the new symbols are declared, bound and exported, and the refusals that need no
device refuse.  No compute."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import bam_records as br
import bam_write_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFQ_ERR_INVALID = -1
GOLDEN = os.path.join(ROOT, "tests", "golden", "bam_write.json")
# the golden's commands: `what`, and the mode of the indel qualities
COMMANDS = {"viterbi": (wm.VITERBI, None), "viterbi_k": (wm.VITERBI_K, None), "alnqual_r": (wm.ALNQUAL_R, None),
            "alnqual": (wm.ALNQUAL, None), "alnqual_r_B": (wm.ALNQUAL_R_NO_BAQ, None), "alnqual_r_A": (wm.ALNQUAL_R_NO_IDAQ, None),
            "alnqual_e": (wm.ALNQUAL, None), "indelqual_uniform": (wm.INDELQUAL, wm.UNIFORM),
            "indelqual_dindel": (wm.INDELQUAL, wm.DINDEL), "chain": (wm.CHAIN, wm.DINDEL)}


def golden_records(rows, ref=b""):
    """the rows of the golden (pos, flag, mapq, l_qname, n_cigar, l_qseq, hex) -> a records dict"""
    datas = [bytes.fromhex(r[6]) for r in rows]
    col = lambda k, dt: np.asarray([r[k] for r in rows], dt)
    return {"data": np.frombuffer(b"".join(datas), np.uint8).copy(),
            "data_off": np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.int64),
            "pos": col(0, np.int32), "flag": col(1, np.uint16), "mapq": col(2, np.uint8), "l_qname": col(3, np.uint16),
            "n_cigar": col(4, np.uint32), "l_qseq": col(5, np.int32), "ref": bytes(ref)}


def results_in(out):
    """what the model takes from the binary's output records: positions, CIGARs, the tag strings it appended (the LAST Z field of
    the tag that is l_qseq long; '?' where there is none) and which reads the alignment step gives ai / ad -- idaq's own count of
    the indels it looks at (bam_md_ext.c:118-120, :180-181): an I of at most 16 bases, a D of at most 16 that is not in front of
    the first query base"""
    n = len(out["pos"])
    cigars = wm.record_cigars(out)
    data = bytes(out["data"])
    tags = {t: [] for t in (b"lb", b"ai", b"ad", b"BI", b"BD")}
    flags = np.zeros(n, np.uint8)
    for r in range(n):
        l, o1 = int(out["l_qseq"][r]), int(out["data_off"][r + 1])
        a = int(out["data_off"][r]) + int(out["l_qname"][r]) + 4 * int(out["n_cigar"][r]) + (l + 1) // 2 + l
        aux = data[a:o1]
        fields = wm.aux_fields(aux)
        for t in tags:
            got = [aux[f[0] + 3:f[1] - 1] for f in fields if f[2] == t and f[3] == "Z" and f[1] - f[0] == l + 4]
            tags[t].append(np.frombuffer(got[-1] if got else b"?" * l, np.uint8))
        y = 0
        for w in cigars[r].tolist():
            op, ln = w & 15, w >> 4
            if op == 1 and ln <= 16:
                flags[r] |= 1
            if op == 2 and ln <= 16 and y > 0:
                flags[r] |= 2
            if op in (0, 1, 4, 7, 8):
                y += ln
    cat = lambda t: np.concatenate(tags[t] + [np.zeros(0, np.uint8)])
    return out["pos"], cigars, cat(b"lb"), cat(b"ai"), cat(b"ad"), flags, cat(b"BI"), cat(b"BD")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("name", sorted(COMMANDS))
def test_model_reproduces_the_binary(golden, name):
    what, idq = COMMANDS[name]
    recs = golden_records(golden["input"])
    want = golden_records(golden["outputs"][name])
    pos, cigars, lb, ai, ad, fl, bi, bd = results_in(want)
    got = wm.rewrite(recs, None, what, pos, cigars, lb, ai, ad, fl, bi, bd, idq)
    for k in ("data_off", "pos", "n_cigar", "flag", "mapq", "l_qname", "l_qseq"):
        assert np.array_equal(got[k], want[k]), (name, k)
    for r in range(len(want["pos"])):
        a = bytes(got["data"][got["data_off"][r]:got["data_off"][r + 1]])
        b = bytes(want["data"][want["data_off"][r]:want["data_off"][r + 1]])
        assert a == b, (name, r, a.hex(), b.hex())


def test_the_golden_holds_the_cases_the_rules_turn_on(golden):
    recs = golden_records(golden["input"])
    data = bytes(recs["data"])
    seen = set()
    kinds = set()
    for r in range(len(recs["pos"])):
        l = int(recs["l_qseq"][r])
        a = int(recs["data_off"][r]) + int(recs["l_qname"][r]) + 4 * int(recs["n_cigar"][r]) + (l + 1) // 2 + l
        fields = [(f[2], f[3]) for f in wm.aux_fields(data[a:int(recs["data_off"][r + 1])])]
        tags = [t for t, _ in fields]
        seen |= {"dup_" + t.decode() for t in tags if tags.count(t) > 1}
        seen |= {"%s_%s" % (t.decode(), y) for t, y in fields if t in (b"lb", b"ai", b"ad", b"BI", b"BD", b"NM", b"AS", b"MC")}
        seen |= {"type_" + y for _, y in fields}
        if tags[:1] == [b"BI"] and fields[0][1] == "i" and (b"BI", "Z") in fields[1:]:
            seen.add("BI_i_in_front_of_BI_Z")
        ops = {w & 15 for w in wm.record_cigars(recs)[r].tolist()}
        kinds.add((1 in ops, 2 in ops))
        if 40 <= l <= 70:
            seen.add("short_reads")
    assert {"dup_NM", "dup_lb", "lb_A", "ai_Z", "ad_A", "BI_i_in_front_of_BI_Z", "short_reads"} <= seen, sorted(seen)
    assert {"type_" + y for y in "AcCsSiIfZHB"} <= seen
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    for bit in (4, 256, 512, 1024):
        assert (recs["flag"] & bit).any(), bit
    vit = golden_records(golden["outputs"]["viterbi"])
    before, after = wm.record_cigars(recs), wm.record_cigars(vit)
    assert sum(1 for r in range(len(recs["pos"])) if not np.array_equal(before[r], after[r])) >= 10     # reads viterbi shifts
    assert (recs["pos"] != vit["pos"]).any() and (recs["n_cigar"] != vit["n_cigar"]).any()
    chain = golden_records(golden["outputs"]["chain"])
    assert not np.array_equal(chain["data_off"], recs["data_off"])


def test_the_model_on_hand_made_records():
    """the rules where the golden cannot isolate them: which field of a tag goes, what stays in which order, what is appended"""
    x, nm, nm2 = br.aux_field("XA", "c", b"\7"), br.aux_field("NM", "i", b"\1\0\0\0"), br.aux_field("NM", "C", b"\2")
    lb_a, lb_z = br.aux_field("lb", "A", b"L"), br.aux_field("lb", "Z", b"old")
    base = b"q\0" + np.asarray([3 << 4 | 0, 1 << 4 | 1, 1 << 4 | 0], "<u4").tobytes() + bytes(3) + bytes(5)    # 3M1I1M, 5 bases
    cig = np.asarray([3 << 4 | 0, 1 << 4 | 1, 1 << 4 | 0], np.uint32)
    one = lambda aux, what, flag=0, fl=1, idq=None: wm.rewrite_one(base + aux, 2, 3, 5, flag, what, cig, b"LLLLL", b"IIIII", b"DDDDD",
                                                                   fl, b"iiiii", b"ddddd", idq)[len(base):]
    LB, AI, BI, BD = b"lbZLLLLL\0", b"aiZIIIII\0", b"BIZiiiii\0", b"BDZddddd\0"
    assert one(nm + x + nm2, wm.DROP_ALN_TAGS) == x + nm2                             # the first NM only, the second stays
    assert one(nm + x + nm2, wm.DROP_ALN_TAGS, flag=4) == x + nm2                     # unmapped reads included
    assert one(lb_a + x, wm.ALNQUAL_R) == lb_a + x + AI                               # a non-Z lb is neither deleted nor replaced
    assert one(lb_z + x, wm.ALNQUAL_R) == x + LB + AI
    assert one(lb_z + x, wm.ALNQUAL) == lb_z + x + AI                                 # kept, and counted as present
    assert one(lb_z + br.aux_field("ai", "Z", b"o"), wm.ALNQUAL) == lb_z + br.aux_field("ai", "Z", b"o")    # everything there
    assert one(br.aux_field("ai", "Z", b"o"), wm.ALNQUAL) == br.aux_field("ai", "Z", b"o") + LB + AI         # ai twice, as the reference
    assert one(lb_z, wm.ALNQUAL_R, flag=4) == lb_z                                    # passes through
    assert one(x, wm.ALNQUAL_R, fl=0) == x + LB                                       # the read got no ai tag
    assert one(br.aux_field("BI", "i", b"\1\0\0\0") + br.aux_field("BI", "Z", b"o") + x, wm.INDELQUAL, idq=wm.UNIFORM) \
        == br.aux_field("BI", "Z", b"o") + x + BI + BD
    assert one(x, wm.INDELQUAL, flag=1024, idq=wm.DINDEL) == x and one(x, wm.INDELQUAL, flag=1024, idq=wm.UNIFORM) == x + BI + BD
    assert one(nm + lb_z, wm.CHAIN, idq=wm.DINDEL) == LB + AI + BI + BD
    with pytest.raises(ValueError):
        one(b"XZZabc", wm.DROP_ALN_TAGS)


def test_edge_table_rows_are_well_formed():
    chunks = br.source_constant("LFQ_BAM_COPY_CHUNKS")
    cases = wm.edge_cases()
    assert len(cases) > 40
    for name, row in cases.items():
        recs = br.encode(row["reads"], ref=wm.REF, **row["kw"])
        cigars = wm.record_cigars(recs) if row["set_cigar"] is None else [
            np.asarray([(ln << 4) | br.OPS.index(o) for o, ln in row["set_cigar"](i)], np.uint32) for i in range(len(row["reads"]))]
        nb = int(recs["l_qseq"].sum())
        fill = np.full(nb, 70, np.uint8)
        out = wm.rewrite(recs, None, row["what"], recs["pos"], cigars, fill, fill, fill, np.full(len(cigars), 3, np.uint8), fill, fill,
                         row["idq"])
        assert out["data_off"][-1] == len(out["data"]) > 0, name
    recs = br.encode(cases["record_longer_than_a_tile"]["reads"], ref=wm.REF)
    assert int(np.diff(recs["data_off"]).max()) > 16 * chunks
    row = cases["output_records_at_every_offset_mod_16"]
    recs = br.encode(row["reads"], ref=wm.REF, **row["kw"])
    out = wm.rewrite(recs, None, row["what"], recs["pos"], wm.record_cigars(recs), None, None, None, None,
                     np.full(int(recs["l_qseq"].sum()), 70, np.uint8), np.full(int(recs["l_qseq"].sum()), 71, np.uint8), row["idq"])
    assert set((out["data_off"][:-1] % 16).tolist()) == set(range(16))
    row = cases["appended_fields_straddle_chunks_and_tiles"]
    recs = br.encode(row["reads"], ref=wm.REF, **row["kw"])
    nb, tile = int(recs["l_qseq"].sum()), 16 * chunks
    out = wm.rewrite(recs, None, row["what"], recs["pos"], wm.record_cigars(recs), None, None, None, None, np.full(nb, 70, np.uint8),
                     np.full(nb, 71, np.uint8), row["idq"])
    ends, ls = out["data_off"][1:], recs["l_qseq"].astype(np.int64)
    heads = np.concatenate([ends - 2 * (ls + 4), ends - (ls + 4)])       # where the heads of BI and BD lie in the blob
    assert set((heads % 16).tolist()) == set(range(16))
    assert ((heads % tile) > tile - 3).any()                # a 3-byte head cut by a tile's end
    assert (heads // tile != (np.concatenate([ends - (ls + 4), ends]) - 1) // tile).sum() >= 2      # fields across a tile's end


def test_the_new_symbols_are_declared_bound_and_exported():
    from lofreq_amd import _lib, pileup
    import lofreq_amd as la
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    assert re.search(r"int lfq_readset_encode_bam\(lfq_ctx \*ctx, lfq_readset \*rs, const lfq_bam_records \*recs, "
                     r"const int64_t \*src_or_null,\s*unsigned what, const lfq_bam_encoded \*\*out\);", hdr)
    assert "int lfq_last_bam_encode_times(lfq_ctx *ctx, lfq_bam_encode_times *t);" in hdr
    for name in ("lfq_readset_encode_bam", "lfq_last_bam_encode_times"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    vp = C.c_void_p
    assert L.lfq_readset_encode_bam.argtypes == [vp, vp, C.POINTER(_lib.BamRecords), vp, C.c_uint, C.POINTER(C.POINTER(_lib.BamEncoded))]
    assert L.lfq_last_bam_encode_times.argtypes == [vp, C.POINTER(_lib.BamEncodeTimes)]
    assert C.sizeof(_lib.BamEncoded) == 48 and C.sizeof(_lib.BamEncodeTimes) == 56 and C.sizeof(_lib.BamRecords) == 88
    consts = {"LFQ_BAM_PUT_ALIGNMENT": 1, "LFQ_BAM_DROP_ALN_TAGS": 2, "LFQ_BAM_PUT_LB": 4, "LFQ_BAM_PUT_IDAQ": 8,
              "LFQ_BAM_KEEP_EXISTING": 16, "LFQ_BAM_PUT_INDELQUAL": 32}
    for k, v in consts.items():
        assert int(re.search(r"#define %s\s+(\d+)" % k, hdr).group(1)) == v == getattr(_lib, k) == getattr(la, k)
        assert k in la.__all__
    assert (wm.PUT_ALIGNMENT, wm.DROP_ALN_TAGS, wm.PUT_LB, wm.PUT_IDAQ, wm.KEEP_EXISTING, wm.PUT_INDELQUAL) == (1, 2, 4, 8, 16, 32)
    assert (wm.UNIFORM, wm.DINDEL) == (_lib.LFQ_IDQ_UNIFORM, _lib.LFQ_IDQ_DINDEL)
    assert callable(pileup.ReadSet.encode_bam) and callable(la.last_bam_encode_times) and "last_bam_encode_times" in la.__all__
    assert int(re.search(r"#define LFQ_ABI_VERSION (\d+)", hdr).group(1)) == 10 and L.lfq_abi_version() == 10


def _records(recs, **change):
    from lofreq_amd import _lib
    a = dict(recs, **change)
    rc = _lib.BamRecords()
    rc.n_reads = a.get("n_reads", len(recs["pos"]))
    for k in ("data", "data_off", "pos", "flag", "mapq", "l_qname", "n_cigar", "l_qseq"):
        setattr(rc, k, None if a[k] is None else a[k].ctypes.data)
    return rc, a                                            # (a keeps the arrays alive)


def test_host_checked_refusals_need_no_device():
    """the refusals that are decided before the read set is looked at, and the read set of another context -- with zeroed buffers
    where a context and a read set would lie: a call that went on to the device would not come back with LFQ_ERR_INVALID"""
    from lofreq_amd import _lib
    L = _lib.load()
    recs = br.encode([br.mk(9, 1), br.mk(12, 2), br.mk(5, 3, tags=None)])
    bogus, bogus_rs = C.create_string_buffer(4096), C.create_string_buffer(4096)
    ctx, rs = C.cast(bogus, C.c_void_p), C.cast(bogus_rs, C.c_void_p)
    enc = lambda c, s, r, what, o: L.lfq_readset_encode_bam(c, s, None if r is None else C.byref(r), None, what, o)
    out = C.POINTER(_lib.BamEncoded)()
    rc, keep = _records(recs)
    for c, s, r, o in ((None, rs, rc, C.byref(out)), (ctx, None, rc, C.byref(out)), (ctx, rs, None, C.byref(out)), (ctx, rs, rc, None)):
        assert enc(c, s, r, wm.VITERBI, o) == LFQ_ERR_INVALID
    for what in (0, 64, 1 << 31, wm.VITERBI | 128, wm.KEEP_EXISTING, wm.KEEP_EXISTING | wm.VITERBI | wm.INDELQUAL):
        out = C.cast(C.c_void_p(0xdead0), C.POINTER(_lib.BamEncoded))
        assert enc(ctx, rs, rc, what, C.byref(out)) == LFQ_ERR_INVALID, what
        assert not out                                      # *out = NULL
    rc, keep = _records(recs, n_reads=-1)
    assert enc(ctx, rs, rc, wm.VITERBI, C.byref(out)) == LFQ_ERR_INVALID
    for k in ("data", "data_off", "pos", "flag", "mapq", "l_qname", "n_cigar", "l_qseq"):
        rc, keep = _records(recs, **{k: None})
        assert enc(ctx, rs, rc, wm.VITERBI, C.byref(out)) == LFQ_ERR_INVALID, k
    off = recs["data_off"].copy()
    off[1], off[2] = off[2], off[1]
    rc, keep = _records(recs, data_off=off)
    assert enc(ctx, rs, rc, wm.VITERBI, C.byref(out)) == LFQ_ERR_INVALID                # decreasing data_off
    lq = recs["l_qseq"].copy()
    lq[1] = -1
    rc, keep = _records(recs, l_qseq=lq)
    assert enc(ctx, rs, rc, wm.VITERBI, C.byref(out)) == LFQ_ERR_INVALID                # l_qseq < 0
    for k, add in (("l_qseq", 40), ("n_cigar", 30), ("l_qname", 200)):                  # a record shorter than its fields
        a = recs[k].copy()
        a[2] += add
        rc, keep = _records(recs, **{k: a})
        assert enc(ctx, rs, rc, wm.VITERBI, C.byref(out)) == LFQ_ERR_INVALID, k
    off = recs["data_off"].copy()
    off[3] += 1 << 31
    rc, keep = _records(recs, data_off=off)
    assert enc(ctx, rs, rc, wm.VITERBI, C.byref(out)) == LFQ_ERR_INVALID                # a record of 2^31 bytes
    rc, keep = _records(recs)
    assert enc(ctx, rs, rc, wm.VITERBI, C.byref(out)) == LFQ_ERR_INVALID                # the read set is not this context's
    t = _lib.BamEncodeTimes()
    assert L.lfq_last_bam_encode_times(None, C.byref(t)) == LFQ_ERR_INVALID and L.lfq_last_bam_encode_times(ctx, None) == LFQ_ERR_INVALID
