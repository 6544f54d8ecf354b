"""-m gpu: the lb / ai / ad tags a BAM already carries -- lfq_readset_create_from_bam_tags, lfq_readset_fetch_stored_tags,
lfq_readset_baq_fill, lfq_region_set_reuse_tags -- against the model of tests/tag_reuse_model.py (held to the 2.1.4 binary by
test_tag_reuse_model.py), the plain lfq_readset_baq on the same reads, the array road of lfq_readset_create, and the VCFs of the
binary in tests/golden/tag_reuse.json."""
import ctypes as C
import json

import numpy as np
import pytest

import bam_records as br
import baq_edges as be
import tag_reuse_model as trm
from test_tag_reuse_model import FIXTURE, stored_edge_cases, unusable_cases

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

LFQ_ERR_INVALID = -1
REF = ("ACGTTGCAAGGCTTAACCGGATCGATTACAGGCATCGAGCTA" * 12).encode()
CASES = stored_edge_cases()
BOTH = trm.READ_LB | trm.READ_IDAQ


def _from(la, caller, recs, read_tags=0):
    return la.ReadSet.from_bam_records(caller, recs["data"], recs["data_off"], recs["pos"], recs["flag"], recs["mapq"],
                                       recs["l_qname"], recs["n_cigar"], recs["l_qseq"], recs["ref"], read_tags=read_tags)


def _records_struct(recs, ref):
    from lofreq_amd import _lib
    rc = _lib.BamRecords()
    rc.n_reads = len(recs["pos"])
    for k in ("data", "data_off", "pos", "flag", "mapq", "l_qname", "n_cigar", "l_qseq"):
        setattr(rc, k, recs[k].ctypes.data)
    rc.ref = C.cast(C.c_char_p(ref), C.c_void_p)
    rc.ref_len = len(ref)
    return rc


def _same_bytes(name, got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    assert len(got) == len(want) and bad.size == 0, (name, bad[:8], np.asarray(got)[bad[:8]], np.asarray(want)[bad[:8]])


def _check_bases(rs, recs):
    """BI / BD, bases and qualities are what the plain decode gives"""
    E = br.expected_arrays(recs)
    seq, qual, bi, bd, fl = rs.fetch_bases()
    assert np.array_equal(fl, E["flags"])
    for name, got in (("seq", seq), ("qual", qual), ("bi", bi), ("bd", bd)):
        _same_bytes(name, got, E[name])


# ---- 1. the decode ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_stored_tags_equal_the_model(caller, name):
    import lofreq_amd as la
    reads, kw = CASES[name]
    recs = br.encode(reads, ref=REF, **kw)
    E = trm.stored_tags(recs)
    rs = _from(la, caller, recs, BOTH)
    lb, ai, ad, fl = rs.fetch_stored_tags()
    assert np.array_equal(fl, E["flags"])
    for t, got in (("lb", lb), ("ai", ai), ("ad", ad)):
        _same_bytes(t, got, E[t])
    _check_bases(rs, recs)
    assert la.last_bam_decode_times(caller)["n_launches"] == (3 if E["flags"].any() else 2)
    rs.close()
    only = trm.stored_tags(recs, trm.READ_IDAQ)             # one of the two bits: the other tag is not looked at
    rs = _from(la, caller, recs, trm.READ_IDAQ)
    lb, ai, ad, fl = rs.fetch_stored_tags()
    assert np.array_equal(fl, only["flags"]) and (lb == 33).all()
    _same_bytes("ai", ai, only["ai"])
    _same_bytes("ad", ad, only["ad"])
    rs.close()


def test_no_read_tagged_is_the_plain_decode(caller):
    import lofreq_amd as la
    reads, kw = CASES["no_read_tagged"]
    recs = br.encode(reads, ref=REF, **kw)
    a, b = _from(la, caller, recs, BOTH), _from(la, caller, recs)
    for x, y in zip(a.fetch_bases(), b.fetch_bases()):
        assert np.array_equal(x, y)
    for x, y in zip(a.fetch_stored_tags(), b.fetch_stored_tags()):
        assert np.array_equal(x, y)
    assert not a.fetch_stored_tags()[3].any() and (a.fetch_stored_tags()[0] == 33).all()
    a.baq_fill(idaq=True)                                   # nothing stored: the call is lfq_readset_baq
    b.baq(idaq=True)
    for x, y in zip(a.fetch_tags(idaq=True), b.fetch_tags(idaq=True)):
        assert np.array_equal(x, y)
    st = la.last_baq_fill_stats(caller)
    assert st["n_need_hmm"] == st["n_reads"] == len(reads) and st["n_stored_lb"] == 0
    a.close()
    b.close()


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------------

def _refused(caller, aux, read_tags=BOTH):
    import lofreq_amd as la
    from lofreq_amd import _lib
    bad = br.mk(21, 3, tags=None)
    bad["aux_raw"] = aux
    recs = br.encode([br.mk(8, 1), bad, br.mk(13, 2)], ref=REF)        # the refused record is followed by a valid one
    rc = _records_struct(recs, REF)
    out = C.c_void_p(0xdead)
    assert _lib.load().lfq_readset_create_from_bam_tags(caller.h, C.byref(rc), read_tags, C.byref(out)) == LFQ_ERR_INVALID
    assert out.value is None
    good = br.encode([br.mk(8, 1), stored_edge_cases()["l_qseq_17_every_subset"][0][7], br.mk(13, 2)], ref=REF)
    rs = _from(la, caller, good, BOTH)                      # the next call on the context succeeds
    E = trm.stored_tags(good)
    lb, ai, ad, fl = rs.fetch_stored_tags()
    assert np.array_equal(fl, E["flags"]) and fl[1] == 7
    _same_bytes("lb", lb, E["lb"])
    rs.close()
    return recs


@pytest.mark.parametrize("name", sorted(unusable_cases()))
def test_unusable_first_field_is_refused_and_the_context_stays_usable(caller, name):
    import lofreq_amd as la
    recs = _refused(caller, unusable_cases()[name])
    for tags in (0, trm.READ_IDAQ):                         # not selected: not looked at
        rs = _from(la, caller, recs, tags)
        assert not rs.fetch_stored_tags()[3].any()
        rs.close()


@pytest.mark.parametrize("name", sorted(br.malformed_cases()))
def test_malformed_aux_is_still_refused(caller, name):
    _refused(caller, br.aux_field("lb", "Z", bytes([50]) * 21) + br.malformed_cases()[name])


# ---- 3. the fill --------------------------------------------------------------------------------------------------------------------------

def _with_tags(r, subset, seed):
    """the read with foreign lb / ai / ad strings (bit 0 / 1 / 2 of subset)"""
    l = len(r["seq"])
    rng = np.random.default_rng(seed)
    aux = b""
    for k, t in enumerate(("lb", "ai", "ad")):
        if subset >> k & 1:
            aux += br.aux_field(t, "Z", (33 + 50 + rng.integers(0, 40, l + k)).astype(np.uint8).tobytes())
    return dict(r, aux_raw=aux, mapq=60, reverse=bool(seed & 1))


def _shape_batch():
    """every subset of stored tags on the four CIGAR shapes"""
    shapes = ("100M", "50M2I48M", "50M1D50M", "30M1I30M2D39M")
    return [_with_tags(be.make_read("s%d_%d" % (k, s), 1400 + 7 * k + s, cg, seed=10 * k + s), s, 100 * k + s)
            for k, cg in enumerate(shapes) for s in range(8)]


def _route_batch(route):
    """reads of one BAQ route, needing and skipped ones interleaved: full tags, none, lb only in turn"""
    mk = {"narrow plain": lambda i: be.plain("np%d" % i, 300 + 5 * i, 80 + i % 9, seed=i),
          "narrow indel": lambda i: be.make_read("ni%d" % i, 320 + 5 * i, [("M", 40 + i % 7), ("ID"[i % 2], 1), ("M", 50)], seed=i),
          "band8": lambda i: be.make_read("b8%d" % i, 330 + 3 * i, [("M", 40 + i % 11), ("D", 2 + i % 2), ("M", 50)], seed=i),
          "wide": lambda i: be.make_read("w%d" % i, 340 + 3 * i, [("M", 50 + i % 5), ("D", 6 + i % 3), ("M", 45)], seed=i)}[route]
    n = 200 if route in ("narrow plain", "band8") else 24   # more than a wavefront of needing reads where the route has wave-wide state
    reads = [_with_tags(mk(i), (7, 0, 1)[i % 3], i) for i in range(n)]
    want = {"narrow plain": "narrow", "narrow indel": "narrow", "band8": "band8", "wide": "wide"}[route]
    assert all(be.read_geometry(r, be.REF_LEN).route == want for r in reads)
    return reads


def _edge_batch(which):
    base = [be.make_read("e%d" % i, 500 + 4 * i, [("M", 40), ("ID"[i % 2], 1 + i % 2), ("M", 45)] if i % 3 == 0 else [("M", 90)], seed=i)
            for i in range(67)]
    need = {"first": lambda i: i == 0, "last": lambda i: i == len(base) - 1, "none": lambda i: False, "all": lambda i: True}[which]
    # a read that needs the HMM lacks lb; in the batch where all do, some still carry ai / ad for the merge pass
    return [_with_tags(r, ((0, 2, 4, 6)[i % 4] if which == "all" else 0) if need(i) else 7, i) for i, r in enumerate(base)]


BATCHES = {"shapes": _shape_batch, "route narrow plain": lambda: _route_batch("narrow plain"),
           "route narrow indel": lambda: _route_batch("narrow indel"), "route band8": lambda: _route_batch("band8"),
           "route wide": lambda: _route_batch("wide"), "only the first needs": lambda: _edge_batch("first"),
           "only the last needs": lambda: _edge_batch("last"), "none needs": lambda: _edge_batch("none"),
           "all need": lambda: _edge_batch("all")}
_computed = {}


def _batch(la, caller, name):
    """(reads, records, stored tags of the model, what plain lfq_readset_baq computes on the reads decoded without tags) -- the
    reference of a batch is computed once"""
    if name not in _computed:
        reads = BATCHES[name]()
        recs = br.encode(reads, ref=be.CONTIG)
        rs = _from(la, caller, recs)
        rs.baq(extended=True, idaq=True)
        lb, ai, ad, fl = rs.fetch_tags(idaq=True)
        rs.close()
        nb = int(recs["l_qseq"].sum())
        for a in (lb, ai, ad, fl):
            a.setflags(write=False)
        _computed[name] = (reads, recs, trm.stored_tags(recs), {"lb": lb[:nb], "ai": ai[:nb], "ad": ad[:nb], "flags": fl[: len(reads)]})
    return _computed[name]


@pytest.mark.parametrize("redo", (False, True), ids=("keep_lb", "redo_baq"))
@pytest.mark.parametrize("idaq", (False, True), ids=("lb_only", "idaq"))
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_fill_equals_the_model_over_plain_baq(caller, name, idaq, redo):
    import lofreq_amd as la
    reads, recs, stored, computed = _batch(la, caller, name)
    before = caller.baq_times()
    seq_off = np.concatenate([[0], np.cumsum(recs["l_qseq"])])
    lb, ai, ad, fl, need = trm.merge(seq_off, [r["cigar"] for r in reads], stored, computed, idaq, redo)
    rs = _from(la, caller, recs, BOTH)
    rs.baq_fill(extended=True, idaq=idaq, redo_baq=redo)
    g_lb, g_ai, g_ad, g_fl = rs.fetch_tags(idaq=idaq)
    nb = int(seq_off[-1])
    _same_bytes("lb", g_lb[:nb], lb)
    if idaq:
        _same_bytes("ai", g_ai[:nb], ai)
        _same_bytes("ad", g_ad[:nb], ad)
        assert np.array_equal(g_fl[: len(reads)], fl)
    st = la.last_baq_fill_stats(caller)
    eff = np.array([trm.effective_bits(int(s), idaq, redo) for s in stored["flags"]])
    assert st["n_reads"] == len(reads) and st["n_need_hmm"] == int(need.sum())
    assert (st["n_stored_lb"], st["n_stored_ai"], st["n_stored_ad"]) == tuple(int((eff >> k & 1).sum()) for k in range(3))
    if need.any():
        assert st["n_hmm_launches"] >= 1 and caller.baq_times()["n_reads"] == int(need.sum())
    else:                                                   # no HMM kernel, and the BAQ times are left as they were
        assert st["n_hmm_launches"] == 0 and st["ms_hmm"] == 0.0 and caller.baq_times() == before
    if name == "none needs":
        assert need.any() == redo
    if name == "all need":                                  # no read has a stored lb: lb is plain lfq_readset_baq's
        _same_bytes("lb", g_lb[:nb], computed["lb"])
        assert need.all()
    # plain lfq_readset_baq on the same read set recomputes everything and ignores the stored tags
    if idaq:
        rs.baq(extended=True, idaq=True)
        for got, want in zip(rs.fetch_tags(idaq=True), (computed["lb"], computed["ai"], computed["ad"], computed["flags"])):
            _same_bytes("after plain baq", got[: len(want)], want)
    rs.close()


def test_a_second_pass_that_newly_wants_idaq_is_refused(caller):
    import lofreq_amd as la
    from lofreq_amd import _lib
    reads, recs, _, _ = _batch(la, caller, "shapes")
    rs = _from(la, caller, recs, BOTH)
    rs.baq_fill(idaq=False)
    assert _lib.load().lfq_readset_baq_fill(caller.h, rs.h, 1, 1, 0) == LFQ_ERR_INVALID
    rs.baq_fill(idaq=False, redo_baq=True)                  # the same wish again is fine
    rs.close()


# ---- 4. downstream ----------------------------------------------------------------------------------------------------------------------

def test_pileups_of_a_filled_read_set_are_the_array_roads(caller):
    """SNV tracks and indel columns of the filled read set = those of lfq_readset_create given the merged arrays through
    reads->baq and tags->ai / ->ad / ->tag_flags"""
    import lofreq_amd as la
    from test_gpu_maxdepth import _assert_tracks_equal, _tracks_host
    from test_gpu_readset_viterbi import _cols_equal
    fx = json.load(open(FIXTURE))
    reads, recs = trm.fixture_records(fx)
    ref = fx["genome"].encode()
    stored = trm.stored_tags(recs)
    plain = _from(la, caller, recs)
    plain.baq(extended=True, idaq=True)
    c_lb, c_ai, c_ad, c_fl = plain.fetch_tags(idaq=True)
    plain.close()
    seq_off = np.concatenate([[0], np.cumsum(recs["l_qseq"])])
    nb = int(seq_off[-1])
    lb, ai, ad, fl, need = trm.merge(seq_off, [r["cigar"] for r in reads], stored,
                                     {"lb": c_lb[:nb], "ai": c_ai[:nb], "ad": c_ad[:nb], "flags": c_fl}, True, False)
    assert 0 < need.sum() < len(reads)
    arr = []
    for i, r in enumerate(reads):
        a, b = int(seq_off[i]), int(seq_off[i + 1])
        d = {k: r[k] for k in ("pos0", "cigar", "seq", "qual", "mapq", "reverse")}
        d.update(lb=lb[a:b], bi=np.full(b - a, trm.BI_BYTE, np.uint8), bd=np.full(b - a, trm.BD_BYTE, np.uint8),
                 ai=ai[a:b] if fl[i] & 1 else None, ad=ad[a:b] if fl[i] & 2 else None)
        arr.append(d)
    caller.set_pileup_nt_packed(False)
    try:
        filled = _from(la, caller, recs, BOTH)
        filled.baq_fill(extended=True, idaq=True)
        t_a = _tracks_host(caller, filled.pileup_snv(0, len(ref)))
        cols_a, pos_a = filled.pileup_indels(0, len(ref))
        road = la.ReadSet(caller, arr, ref)
        t_b = _tracks_host(caller, road.pileup_snv(0, len(ref)))
        cols_b, pos_b = road.pileup_indels(0, len(ref))
        assert len(t_a["col_pos"]) > 100
        _assert_tracks_equal(t_a, t_b)
        assert np.array_equal(pos_a, pos_b) and sum(len(k) for k in cols_a.keys) > 0
        _cols_equal(cols_a, cols_b)
        filled.close()
        road.close()
    finally:
        caller.set_pileup_nt_packed(True)


def test_encode_and_viterbi_refusals(caller):
    import lofreq_amd as la
    from lofreq_amd import _lib
    L = _lib.load()
    reads, recs, _, _ = _batch(la, caller, "shapes")
    rc = _records_struct(recs, be.CONTIG)
    rs = _from(la, caller, recs, BOTH)
    new = C.c_void_p(0xdead)
    assert L.lfq_readset_viterbi(caller.h, rs.h, -1, C.byref(new), None, None) == LFQ_ERR_INVALID
    assert new.value is None
    rs.baq_fill(extended=True, idaq=True)
    for what in (la.LFQ_BAM_PUT_LB, la.LFQ_BAM_PUT_IDAQ, la.LFQ_BAM_PUT_LB | la.LFQ_BAM_PUT_IDAQ | la.LFQ_BAM_KEEP_EXISTING):
        out = C.POINTER(_lib.BamEncoded)()
        assert L.lfq_readset_encode_bam(caller.h, rs.h, C.byref(rc), None, what, C.byref(out)) == LFQ_ERR_INVALID
    rs.baq(extended=True, idaq=True)                        # the full recompute: alnqual on the device as before
    rs.encode_bam(recs, what=la.LFQ_BAM_PUT_LB | la.LFQ_BAM_PUT_IDAQ)
    rs.close()
    untagged = br.encode([dict(r, aux_raw=b"") for r in reads], ref=be.CONTIG)
    rs = _from(la, caller, untagged, BOTH)                  # no read has a stored tag: every step runs, viterbi included
    new, _, _ = rs.viterbi(-1)
    new.close()
    rs.close()


# ---- 5. the region binding ------------------------------------------------------------------------------------------------------------

def _run_region(caller, lib, fx, mode, road="record", viterbi_first=None):
    """the fixture's records through lfq_region_add_record under lfq_region_set_reuse_tags(mode) -> (VCF lines, conf)"""
    import golden_util as gu
    import lofreq_amd as la
    from test_gpu_chain import _RegionOpts, _bam_fields
    P = C.CDLL(lib)
    reads = trm.fixture_reads(fx)
    ref = fx["genome"].encode()
    kw, _ = gu.conf_kwargs(fx["call_args"])
    conf = la.VarcallConf(**kw)
    lines = []
    EMIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)
    cb = EMIT(lambda user, s: lines.append(s.decode().rstrip("\n")))
    o = _RegionOpts()
    P.lfq_region_opts_init(C.byref(o))
    o.use_idaq = o.call_indels = 1
    h = C.c_void_p()
    P.lfq_region_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, EMIT, C.c_void_p]
    assert P.lfq_region_open(C.byref(h), caller.h, C.byref(conf.c), C.byref(o), cb, None) == 0
    P.lfq_region_set_reuse_tags.argtypes = [C.c_void_p, C.c_int]
    P.lfq_region_set_viterbi.argtypes = [C.c_void_p, C.c_int, C.c_int]
    P.lfq_region_begin.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int64]
    P.lfq_region_add_read.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_char_p, C.c_char_p]
    P.lfq_region_add_record.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
    P.lfq_region_end.argtypes = [C.c_void_p]
    P.lfq_region_close.argtypes = [C.c_void_p, C.c_void_p]
    refusals = []
    if viterbi_first is True:
        assert P.lfq_region_set_viterbi(h, 1, -1) == 0
        refusals.append(P.lfq_region_set_reuse_tags(h, mode))
    elif viterbi_first is False:
        assert P.lfq_region_set_reuse_tags(h, mode) == 0
        refusals.append(P.lfq_region_set_viterbi(h, 1, -1))
        assert P.lfq_region_set_viterbi(h, 0, -1) == 0
    else:
        assert P.lfq_region_set_reuse_tags(h, 3) == LFQ_ERR_INVALID and P.lfq_region_set_reuse_tags(h, -1) == LFQ_ERR_INVALID
        assert P.lfq_region_set_reuse_tags(h, mode) == 0
    if viterbi_first is None:
        assert P.lfq_region_begin(h, b"chr1", ref, len(ref), 0, len(ref)) == 0
        for i, r in enumerate(reads):
            flag = 16 if r["reverse"] else 0
            if road == "record":
                lq, nc, ls, data = br.record_fields(r, len(r["name"]) + 1)
                assert P.lfq_region_add_record(h, r["pos0"], flag, r["mapq"], lq, nc, ls, data, len(data)) == 1
            else:
                seq4, cig, _, _ = _bam_fields(r)
                q = np.asarray(r["qual"], np.uint8)
                refusals.append(P.lfq_region_add_read(h, r["pos0"], flag, r["mapq"], len(cig), cig.ctypes.data, len(q), seq4.ctypes.data,
                                                      q.ctypes.data, None, None))
        assert P.lfq_region_end(h) == 0
    wo = C.c_int64(-1)
    assert P.lfq_region_close(h, C.byref(wo)) == 0
    return lines, conf, refusals


@pytest.mark.parametrize("mode,key", ((1, "vcf"), (2, "vcf_D"), (0, "vcf_stripped")))
def test_region_modes_reproduce_the_binary_vcfs(caller, tmp_path, mode, key):
    import lofreq_amd as la
    from test_gpu_chain import _build_region_lib, _epilogue
    fx = json.load(open(FIXTURE))
    lib = _build_region_lib(tmp_path)
    lines, conf, _ = _run_region(caller, lib, fx, mode)
    assert conf.num_snv_tests == fx[key]["num_tests"]["snv"] and conf.num_indel_tests == fx[key]["num_tests"]["indel"]
    assert _epilogue(la, lines, conf) == fx[key]["vcf"]
    if mode:
        st = la.last_baq_fill_stats(caller)
        assert st["n_reads"] == len(fx["reads"]) and st["n_stored_ai"] > 0 and st["n_stored_ad"] > 0
        if mode == 1:
            assert 0 < st["n_need_hmm"] < st["n_reads"] and st["n_stored_lb"] > 0
        else:                                               # -D: no stored lb counts, so every read runs the HMM
            assert st["n_need_hmm"] == st["n_reads"] and st["n_stored_lb"] == 0


def test_region_refuses_add_read_and_viterbi_under_a_mode(caller, tmp_path):
    from test_gpu_chain import _build_region_lib
    fx = json.load(open(FIXTURE))
    lib = _build_region_lib(tmp_path)
    _, _, refusals = _run_region(caller, lib, fx, 1, road="read")
    assert refusals and set(refusals) == {LFQ_ERR_INVALID}
    for first in (True, False):
        _, _, refusals = _run_region(caller, lib, fx, 1, viterbi_first=first)
        assert refusals == [LFQ_ERR_INVALID]
