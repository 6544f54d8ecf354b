"""-m gpu: lfq_readset_encode_bam -- the results of a read set's steps written into the bytes of BAM records on the device --
against tests/bam_write_model.py::rewrite (held to the 2.1.4 binary by tests/test_bam_write_model.py), fed with what the read set
itself fetched, at the edges of the plan pass and the copy pass; and the whole chain viterbi -> alnqual -> indelqual -> encode
against the records the binary's own chain wrote."""
import ctypes as C
import json

import numpy as np
import pytest

import bam_records as br
import bam_write_model as wm
from test_bam_write_model import GOLDEN, golden_records

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

LFQ_ERR_INVALID = -1
CASES = wm.edge_cases()
UNIFORM_QUALS = (40, 30)


def _from(la, caller, recs):
    return la.ReadSet.from_bam_records(caller, recs["data"], recs["data_off"], recs["pos"], recs["flag"], recs["mapq"],
                                       recs["l_qname"], recs["n_cigar"], recs["l_qseq"], recs["ref"])


def _steps(rs, baq, idq):
    """the steps a row asks for -> what the read set then holds, as the model takes it"""
    lb = ai = ad = fl = bi = bd = None
    if baq:
        rs.baq(extended=True, idaq=True)
        lb, ai, ad, fl = rs.fetch_tags(idaq=True)
    if idq:
        rs.indelqual("uniform" if idq == wm.UNIFORM else "dindel", *UNIFORM_QUALS)
        bi, bd = rs.fetch_indelquals()
    return lb, ai, ad, fl, bi, bd


def _same_records(got, want):
    for k in ("src", "data_off", "pos", "n_cigar", "flag", "mapq", "l_qname", "l_qseq"):
        assert np.array_equal(got[k], want[k]), (k, got[k][:8], want[k][:8])
        assert got[k].dtype == want[k].dtype, k
    for r in range(len(want["pos"])):
        a = bytes(got["data"][got["data_off"][r]:got["data_off"][r + 1]])
        b = bytes(want["data"][want["data_off"][r]:want["data_off"][r + 1]])
        assert a == b, (r, a.hex(), b.hex())
    assert len(got["data"]) == len(want["data"])


# ---- 1. the edge table ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_edge_table(caller, name):
    import lofreq_amd as la
    row = CASES[name]
    reads, kw = row["reads"], row["kw"]
    n = len(reads)
    recs = br.encode(reads, ref=wm.REF, **kw)
    set_recs, src = recs, None
    if row["set_cigar"] is not None:                        # the read set brings other CIGARs than the records hold
        set_recs = br.encode([dict(r, cigar=row["set_cigar"](i), pos0=r["pos0"] + 1) for i, r in enumerate(reads)], ref=wm.REF, **kw)
    if row["reverse"]:
        set_recs, src = br.encode(reads[::-1], ref=wm.REF, **kw), np.arange(n, dtype=np.int64)[::-1].copy()
    rs = _from(la, caller, set_recs)
    lb, ai, ad, fl, bi, bd = _steps(rs, row["baq"], row["idq"])
    got = rs.encode_bam(recs, src, row["what"])
    want = wm.rewrite(recs, src, row["what"], set_recs["pos"], wm.record_cigars(set_recs), lb, ai, ad, fl, bi, bd, row["idq"])
    _same_records(got, want)
    t = la.last_bam_encode_times(caller)
    assert t["n_launches"] == 2 and t["n_reads"] == n
    assert t["n_in_bytes"] == int(recs["data_off"][-1] - recs["data_off"][0]) and t["n_out_bytes"] == int(want["data_off"][-1])
    if name == "n_cigar_grows":
        assert (got["n_cigar"] > recs["n_cigar"]).all() and (got["pos"] == recs["pos"] + 1).all()
    if name == "n_cigar_shrinks":
        assert (got["n_cigar"] < recs["n_cigar"]).all()
    if row["baq"] and name.startswith("what_alnqual"):
        assert fl.any() and not fl.all()                    # reads with and without ai / ad
    rs.close()


# ---- 2. the round trip and the chain ----------------------------------------------------------------------------------------------

def test_round_trip_through_the_decode(caller):
    """from_bam_records(encode_bam(...)): the decode finds the BI / BD the encode wrote, and bases and qualities are unchanged"""
    import lofreq_amd as la
    reads = CASES["what_chain"]["reads"]
    reads = [r for r in reads if not r["flag_other"] & 0x704]           # (Dindel mode writes no BI / BD into the others)
    recs = br.encode(reads, ref=wm.REF)
    rs = _from(la, caller, recs)
    seq, qual, _, _, _ = rs.fetch_bases()
    rs.indelqual("dindel")
    bi, bd = rs.fetch_indelquals()
    out = rs.encode_bam(recs, None, wm.INDELQUAL | wm.DROP_ALN_TAGS)
    back = _from(la, caller, out)
    seq2, qual2, bi2, bd2, fl2 = back.fetch_bases()
    assert np.array_equal(seq, seq2) and np.array_equal(qual, qual2)
    assert np.array_equal(bi, bi2) and np.array_equal(bd, bd2) and (fl2 == 3).all()
    assert len(set(bi.tolist())) > 1
    rs.close()
    back.close()


def test_the_golden_chain_end_to_end(caller):
    """viterbi -> baq + idaq -> indelqual --dindel -> encode on the device equals, byte for byte, the records that
    `lofreq viterbi | lofreq alnqual -r | lofreq indelqual --dindel` of the 2.1.4 binary wrote: positions, CIGARs, the tags that
    went, and the lb / ai / ad / BI / BD strings"""
    import lofreq_amd as la
    fx = json.load(open(GOLDEN))
    ref = fx["genome"].encode()
    recs = golden_records(fx["input"], ref)
    want = golden_records(fx["outputs"]["chain"], ref)
    rs = _from(la, caller, recs)
    new, _, order = rs.viterbi(-1)
    new.baq(extended=True, idaq=True)
    new.indelqual("dindel")
    got = new.encode_bam(recs, order, wm.CHAIN)
    assert sorted(got["src"].tolist()) == list(range(len(recs["pos"]))) and np.array_equal(got["src"], order)
    assert not np.array_equal(order, np.arange(len(order)))
    for j, s in enumerate(got["src"].tolist()):
        a = bytes(got["data"][got["data_off"][j]:got["data_off"][j + 1]])
        b = bytes(want["data"][want["data_off"][s]:want["data_off"][s + 1]])
        assert a == b, (j, s, a.hex(), b.hex())
        assert got["pos"][j] == want["pos"][s] and got["n_cigar"][j] == want["n_cigar"][s]
        assert got["flag"][j] == want["flag"][s] and got["mapq"][j] == want["mapq"][s]
    rs.close()
    new.close()


@pytest.mark.parametrize("name", ["viterbi", "viterbi_k"])
def test_the_golden_viterbi_commands(caller, name):
    import lofreq_amd as la
    fx = json.load(open(GOLDEN))
    ref = fx["genome"].encode()
    recs = golden_records(fx["input"], ref)
    want = golden_records(fx["outputs"][name], ref)
    rs = _from(la, caller, recs)
    new, _, order = rs.viterbi(-1)
    got = new.encode_bam(recs, order, wm.VITERBI if name == "viterbi" else wm.VITERBI_K)
    for j, s in enumerate(got["src"].tolist()):
        a = bytes(got["data"][got["data_off"][j]:got["data_off"][j + 1]])
        assert a == bytes(want["data"][want["data_off"][s]:want["data_off"][s + 1]]), (j, s)
        assert got["pos"][j] == want["pos"][s] and got["n_cigar"][j] == want["n_cigar"][s]
    rs.close()
    new.close()


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------

def _c_records(recs):
    from lofreq_amd import _lib
    rc = _lib.BamRecords()
    rc.n_reads = len(recs["pos"])
    for k in ("data", "data_off", "pos", "flag", "mapq", "l_qname", "n_cigar", "l_qseq"):
        setattr(rc, k, recs[k].ctypes.data)
    return rc


def _encode_rc(caller, rs, recs, src, what):
    from lofreq_amd import _lib
    out = C.cast(C.c_void_p(0xdead0), C.POINTER(_lib.BamEncoded))
    rc = _c_records(recs)
    code = _lib.load().lfq_readset_encode_bam(caller.h, rs.h, C.byref(rc), None if src is None else src.ctypes.data, what, C.byref(out))
    assert code == 0 or not out
    return code


@pytest.mark.parametrize("name", sorted(br.malformed_cases()))
def test_malformed_aux_is_refused_and_the_context_stays_usable(caller, name):
    import lofreq_amd as la
    good = br.encode([br.mk(8, 1), br.mk(21, 3, tags=None), br.mk(13, 2)], ref=wm.REF)
    bad = br.mk(21, 3, tags=None)
    bad["aux_raw"] = br.malformed_cases()[name]
    recs = br.encode([br.mk(8, 1), bad, br.mk(13, 2)], ref=wm.REF)          # the malformed record is followed by a valid one
    rs = _from(la, caller, good)
    rs.indelqual("uniform", 40)
    assert _encode_rc(caller, rs, recs, None, wm.INDELQUAL) == LFQ_ERR_INVALID
    bi, bd = rs.fetch_indelquals()
    got = rs.encode_bam(good, None, wm.INDELQUAL)
    _same_records(got, wm.rewrite(good, None, wm.INDELQUAL, good["pos"], wm.record_cigars(good), None, None, None, None, bi, bd, wm.UNIFORM))
    rs.close()


def test_refusals_that_need_a_read_set(caller):
    import lofreq_amd as la
    reads = [br.mk(9, 1, tags=None), br.mk(12, 2, tags=None), br.mk(9, 3, tags=None)]
    recs = br.encode(reads, ref=wm.REF)
    rs = _from(la, caller, recs)
    i64 = lambda *v: np.asarray(v, np.int64)
    assert _encode_rc(caller, rs, recs, None, wm.VITERBI) == 0
    assert _encode_rc(caller, rs, br.encode(reads[:2], ref=wm.REF), None, wm.VITERBI) == LFQ_ERR_INVALID        # another n
    for src in (i64(0, 1, 1), i64(0, 1, 3), i64(-1, 1, 2)):                                                     # no permutation
        assert _encode_rc(caller, rs, recs, src, wm.VITERBI) == LFQ_ERR_INVALID
    assert _encode_rc(caller, rs, recs, i64(2, 1, 0), wm.VITERBI) == 0                                          # equal lengths
    assert _encode_rc(caller, rs, recs, i64(1, 0, 2), wm.VITERBI) == LFQ_ERR_INVALID                            # l_qseq differs
    for what in (wm.PUT_LB, wm.PUT_IDAQ, wm.ALNQUAL, wm.INDELQUAL, wm.VITERBI | wm.INDELQUAL):                  # the step has not run
        assert _encode_rc(caller, rs, recs, None, what) == LFQ_ERR_INVALID, what
    rs.baq(extended=True, idaq=False)
    assert _encode_rc(caller, rs, recs, None, wm.PUT_LB) == 0 and _encode_rc(caller, rs, recs, None, wm.PUT_IDAQ) == LFQ_ERR_INVALID
    other = la.SnvCaller(0)
    try:
        from lofreq_amd import _lib
        out = C.POINTER(_lib.BamEncoded)()
        rc = _c_records(recs)
        assert _lib.load().lfq_readset_encode_bam(other.h, rs.h, C.byref(rc), None, wm.VITERBI, C.byref(out)) == LFQ_ERR_INVALID
    finally:
        other.close()
    rs.close()


# ---- 4. the empty batch ---------------------------------------------------------------------------------------------------------------

def test_empty_batch_launches_nothing(caller):
    import lofreq_amd as la
    recs = br.encode([br.mk(5, 1)], ref=wm.REF)
    rs = _from(la, caller, recs)
    rs.encode_bam(recs, None, wm.VITERBI)                   # (so that the times are not zero from the start)
    rs.close()
    assert la.last_bam_encode_times(caller)["n_launches"] == 2
    recs = br.encode([], ref=wm.REF)
    rs = _from(la, caller, recs)
    got = rs.encode_bam(recs, None, wm.VITERBI)
    t = la.last_bam_encode_times(caller)
    assert t["n_launches"] == 0 and t["n_reads"] == 0 and t["n_in_bytes"] == 0 and t["n_out_bytes"] == 0
    assert len(got["data"]) == 0 and got["data_off"].tolist() == [0] and len(got["pos"]) == 0 and len(got["src"]) == 0
    rs.close()
