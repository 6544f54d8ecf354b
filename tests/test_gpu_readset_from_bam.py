"""-m gpu: lfq_readset_create_from_bam / lfq_region_add_record -- BAM records decoded on the device -- against the array road:
the read set must equal, in every observable way, the one lfq_readset_create builds from the arrays the per-base host loop of
lfq_region_add_read makes of the same records (tests/bam_records.py::expected_arrays restates that loop)."""
import ctypes as C

import numpy as np
import pytest

import bam_records as br
import golden_util as gu

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

LFQ_ERR_INVALID = -1
REF = ("ACGTTGCAAGGCTTAACCGGATCGATTACAGGCATCGAGCTA" * 12).encode()
CASES = br.edge_cases()


def _check(rs, recs):
    E = br.expected_arrays(recs)
    seq, qual, bi, bd, fl = rs.fetch_bases()
    assert np.array_equal(rs.seq_off, E["seq_off"])
    assert np.array_equal(fl, E["flags"])
    for name, got in (("seq", seq), ("qual", qual), ("bi", bi), ("bd", bd)):
        bad = np.flatnonzero(got != E[name])
        assert bad.size == 0, (name, bad[:8], got[bad[:8]], E[name][bad[:8]])
    return E


def _from(la, caller, recs):
    return la.ReadSet.from_bam_records(caller, recs["data"], recs["data_off"], recs["pos"], recs["flag"], recs["mapq"],
                                       recs["l_qname"], recs["n_cigar"], recs["l_qseq"], recs["ref"])


# ---- 1. the edge table ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_edge_table(caller, name):
    import lofreq_amd as la
    reads, kw = CASES[name]
    recs = br.encode(reads, ref=REF, **kw)
    if name == "bd_nul_is_the_last_byte":
        assert recs["data"][-1] == 0 and recs["data"][-2] != 0 and recs["data_off"][-1] == len(recs["data"])
    rs = _from(la, caller, recs)
    E = _check(rs, recs)
    t = la.last_bam_decode_times(caller)
    assert t["n_launches"] == 2 and t["n_reads"] == len(reads) and t["n_bases"] == int(E["seq_off"][-1])
    assert t["n_data_bytes"] == int(recs["data_off"][-1] - recs["data_off"][0])
    rs.close()


def test_the_per_read_arrays_and_tag_arrays_are_the_array_roads(caller):
    """what fetch_bases cannot show: positions, CIGARs, mapq, strand and WHICH tag arrays the read set has -- through the indel
    pileup (it reads all of them) on a batch in which only the last read carries BI, beside the array road on expected_arrays"""
    import lofreq_amd as la
    from test_gpu_readset_viterbi import _cols_equal
    reads, kw = CASES["only_the_last_read_has_bi"]
    reads = sorted(reads, key=lambda r: r["pos0"])
    recs = br.encode(reads, ref=REF, **kw)
    E = br.expected_arrays(recs)
    assert E["any_bi"] and not E["any_bd"]
    rs = _from(la, caller, recs)
    R = dict(E, n=len(reads), ref=REF, bd=None)
    ref_set = la.ReadSet.from_arrays(caller, R)
    a, pa = rs.pileup_indels(0, len(REF))
    b, pb = ref_set.pileup_indels(0, len(REF))
    assert np.array_equal(pa, pb) and a.ncols > 50
    _cols_equal(a, b)
    rs.close()
    ref_set.close()


# ---- 2. malformed aux fields: refused by the decode, nothing read beyond a record ---------------------------------------------

@pytest.mark.parametrize("name", sorted(br.malformed_cases()))
def test_malformed_aux_is_refused_and_the_context_stays_usable(caller, name):
    import lofreq_amd as la
    from lofreq_amd import _lib
    bad = br.mk(21, 3, tags=None)
    bad["aux_raw"] = br.malformed_cases()[name]
    recs = br.encode([br.mk(8, 1), bad, br.mk(13, 2)], ref=REF)        # the malformed record is followed by a valid one
    rc = _lib.BamRecords()
    rc.n_reads = 3
    for k in ("data", "data_off", "pos", "flag", "mapq", "l_qname", "n_cigar", "l_qseq"):
        setattr(rc, k, recs[k].ctypes.data)
    rc.ref = C.cast(C.c_char_p(REF), C.c_void_p)
    rc.ref_len = len(REF)
    out = C.c_void_p(0xdead)
    assert _lib.load().lfq_readset_create_from_bam(caller.h, C.byref(rc), C.byref(out)) == LFQ_ERR_INVALID
    assert out.value is None
    good = br.encode([br.mk(8, 1), br.mk(21, 3), br.mk(13, 2)], ref=REF)
    rs = _from(la, caller, good)
    _check(rs, good)
    rs.close()


# ---- 3. the region binding fed with records ---------------------------------------------------------------------------------------

def _run_regions(caller, lib, reads, ref, regions, conf, road, call_indels=True):
    """test_gpu_chain.py::_run_regions with the reads handed over by lfq_region_add_read ("read"), as records by
    lfq_region_add_record ("record"), or alternating ("mixed": -> the return code of the first refused call)"""
    from test_gpu_chain import _RegionOpts, _bam_fields
    P = C.CDLL(lib)
    lines = []
    EMIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)
    cb = EMIT(lambda user, s: lines.append(s.decode().rstrip("\n")))
    o = _RegionOpts()
    P.lfq_region_opts_init(C.byref(o))
    o.use_idaq = o.call_indels = 1 if call_indels else 0
    h = C.c_void_p()
    P.lfq_region_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, EMIT, C.c_void_p]
    assert P.lfq_region_open(C.byref(h), caller.h, C.byref(conf.c), C.byref(o), cb, None) == 0
    P.lfq_region_begin.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int64]
    P.lfq_region_add_read.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_char_p, C.c_char_p]
    P.lfq_region_add_record.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
    P.lfq_region_end.argtypes = [C.c_void_p]
    P.lfq_region_close.argtypes = [C.c_void_p, C.c_void_p]
    taken, refused = 0, None
    for beg, end in regions:
        assert P.lfq_region_begin(h, b"chr1", ref, len(ref), beg, end) == 0
        k = 0
        for i, r in enumerate(reads):
            rlen = sum(l for op, l in r["cigar"] if op in "MDN=X")
            if r["pos0"] >= end or r["pos0"] + rlen <= beg:
                continue
            flag = 16 if r["reverse"] else 0
            if road == "record" or (road == "mixed" and k % 2 == 1):
                lq, nc, ls, data = br.record_fields(dict(r, name="read%d" % i))
                rc = P.lfq_region_add_record(h, r["pos0"], flag, r["mapq"], lq, nc, ls, data, len(data))
            else:
                seq4, cig, bi, bd = _bam_fields(r)
                q = np.asarray(r["qual"], np.uint8)
                rc = P.lfq_region_add_read(h, r["pos0"], flag, r["mapq"], len(cig), cig.ctypes.data, len(q), seq4.ctypes.data,
                                           q.ctypes.data, bi, bd)
            k += 1
            if road == "mixed" and rc < 0:                  # (the region stays with the function that fed it first)
                refused = rc if refused is None else refused
                assert rc == refused
                continue
            assert rc in (0, 1)
            taken += rc
        assert P.lfq_region_end(h) == 0
    wo = C.c_int64(-1)
    assert P.lfq_region_close(h, C.byref(wo)) == 0
    return lines, taken, wo.value, refused


@pytest.mark.parametrize("path", gu.chain_fixtures(), ids=lambda p: p.split("/")[-1])
def test_chain_fixtures_through_add_record(caller, tmp_path, path):
    """the fixtures and regions of test_gpu_chain.py::test_region_binding_snv_fixtures: the VCF lines of the record road are
    the golden's, byte for byte those of the read road, and conf ends with the same factors and counters"""
    import json
    import lofreq_amd as la
    from test_gpu_chain import _build_region_lib, _epilogue
    lib = _build_region_lib(tmp_path)
    fx = json.load(open(path))
    reads = [{"pos0": r[0], "cigar": gu.parse_cigar(r[3]), "seq": la.encode_seq(r[4]),
              "qual": np.array([ord(c) - 33 for c in r[5]], np.uint8), "mapq": r[2], "reverse": bool(r[1] & 16)}
             for r in fx["reads"]]
    ref = fx["genome"].encode()
    kw, ndf = gu.conf_kwargs(fx["call_args"])
    n = len(ref)
    regions = [(0, n // 2), (n // 2, n)]
    got = {}
    for road in ("read", "record"):
        conf = la.VarcallConf(**kw)
        lines, taken, _, _ = _run_regions(caller, lib, reads, ref, regions, conf, road, call_indels=False)
        got[road] = (lines, taken, conf.num_snv_tests, conf.num_indel_tests, conf.bonf_subst, conf.bonf_indel)
        assert conf.num_snv_tests == fx["num_snv_tests"]
        vcf = _epilogue(la, lines, conf)
        if not ndf:
            vcf = [l for l in vcf if l in set(fx["vcf"])]
        assert vcf == fx["vcf"], road
    assert got["record"] == got["read"]
    conf = la.VarcallConf(**kw)
    _, _, _, refused = _run_regions(caller, lib, reads, ref, regions, conf, "mixed", call_indels=False)
    assert refused == LFQ_ERR_INVALID


def test_indel_fixture_with_bi_bd_through_add_record(caller, tmp_path):
    """records that carry BI / BD: the region's "no read came with BI or BD" is what the decode found, and the VCF of
    `lofreq call --call-indels` comes out as the golden has it"""
    import lofreq_amd as la
    from test_gpu_chain import _build_region_lib, _epilogue
    lib = _build_region_lib(tmp_path)
    fx, reads = gu.load_plpindel(gu.plpindel_fixtures()[0], with_alnqual_tags=False)
    ref = fx["genome"].encode()
    kw, _ = gu.conf_kwargs(fx["call_args"])
    n = len(ref)
    conf = la.VarcallConf(**kw)
    lines, taken, wo, _ = _run_regions(caller, lib, reads, ref, [(0, n // 3), (n // 3, n // 3 + 37), (n // 3 + 37, n)], conf, "record")
    assert taken >= len(reads) and wo == 0
    assert conf.num_snv_tests == fx["all"]["num_tests"]["snv"] and conf.num_indel_tests == fx["all"]["num_tests"]["indel"]
    assert _epilogue(la, lines, conf) == fx["all"]["vcf"]


# ---- 4. the host views: steps whose host side reads bases and tags --------------------------------------------------------------

def test_host_side_steps_see_the_same_reads(caller):
    import lofreq_amd as la
    from test_gpu_readset_viterbi import _cols_equal, same
    fx, reads = gu.load_plpindel(gu.plpindel_fixtures()[0], with_alnqual_tags=False)
    ref = fx["genome"].encode()
    assert any(r["bi"] is not None for r in reads) and any(op in "ID" for r in reads for op, _ in r["cigar"])
    recs = br.encode([dict(r, name="q%d" % i) for i, r in enumerate(reads)], ref=ref, before=br.one_of_every_type()[:3])
    rs = _from(la, caller, recs)
    _check(rs, recs)
    ref_set = la.ReadSet(caller, reads, ref)
    a, pa = rs.pileup_indels(0, len(ref))
    b, pb = ref_set.pileup_indels(0, len(ref))
    assert np.array_equal(pa, pb) and sum(len(k) for k in a.keys) > 0
    _cols_equal(a, b)
    new_a, res_a, order_a = rs.viterbi(-1)
    new_b, res_b, order_b = ref_set.viterbi(-1)
    assert same(res_a, res_b) and np.array_equal(order_a, order_b)
    rs.close()                                              # the realigned set needs neither the first one nor the records
    recs["data"][:] = 0
    assert same(new_a.fetch_bases(), new_b.fetch_bases())
    a, pa = new_a.pileup_indels(0, len(ref))
    b, pb = new_b.pileup_indels(0, len(ref))
    assert np.array_equal(pa, pb)
    _cols_equal(a, b)
    for s in (new_a, new_b, ref_set):
        s.close()


def test_the_read_set_outlives_the_callers_arrays(caller):
    import lofreq_amd as la
    reads, kw = CASES["tags_behind_every_type"]
    reads = sorted(reads, key=lambda r: r["pos0"])
    recs = br.encode(reads, ref=REF, **kw)
    keep = {k: v.copy() for k, v in recs.items() if isinstance(v, np.ndarray)}
    rs = _from(la, caller, recs)
    for k, v in recs.items():
        if isinstance(v, np.ndarray):
            v[:] = 0                                        # the records and descriptors are the caller's again
    keep["ref"] = REF
    E = br.expected_arrays(keep)
    ref_set = la.ReadSet.from_arrays(caller, dict(E, n=len(reads), ref=REF))
    from test_gpu_readset_viterbi import _cols_equal
    a, pa = rs.pileup_indels(0, len(REF))
    b, pb = ref_set.pileup_indels(0, len(REF))
    assert np.array_equal(pa, pb)
    _cols_equal(a, b)
    rs.close()
    ref_set.close()


# ---- 5. the empty batch -------------------------------------------------------------------------------------------------------------

def test_empty_batch_launches_nothing(caller):
    import lofreq_amd as la
    rs = _from(la, caller, br.encode([br.mk(5, 1)], ref=REF))          # (so that the times are not zero from the start)
    rs.close()
    assert la.last_bam_decode_times(caller)["n_launches"] == 2
    recs = br.encode([], ref=REF)
    rs = _from(la, caller, recs)
    t = la.last_bam_decode_times(caller)
    assert t["n_launches"] == 0 and t["n_reads"] == 0 and t["n_bases"] == 0 and t["n_data_bytes"] == 0
    seq, qual, bi, bd, fl = rs.fetch_bases()
    assert len(seq) == 0 and len(fl) == 0
    rs.close()
