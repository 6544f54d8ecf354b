"""-m gpu: plp_summary's header lines through the read-level binding (integration/lofreq_amd_region.c,
lfq_region_set_summary): the reads of tests/golden/plpsummary_indel.json cut into three regions whose reads overlap the cuts
give the lines the reference's 2.1.4 binary printed, before each region's VCF lines, and the same VCF lines and counters as a
run without the callback -- which launches no summary kernel."""
import ctypes as C

import numpy as np
import pytest

import plpsummary_ref as ref
from test_gpu_chain import _RegionOpts, _bam_fields, _build_region_lib

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


def _run(caller, lib, reads, genome, regions, conf, with_summary):
    """the region loop of test_gpu_chain._run_regions with the summary callback -> every emitted line, tagged "S" / "V" """
    P = C.CDLL(lib)
    out = []
    EMIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)
    cb_vcf = EMIT(lambda user, s: out.append(("V", s.decode())))
    cb_sum = EMIT(lambda user, s: out.append(("S", s.decode())))
    o = _RegionOpts()
    P.lfq_region_opts_init(C.byref(o))
    o.use_idaq, o.call_indels = 1, 1
    h = C.c_void_p()
    P.lfq_region_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, EMIT, C.c_void_p]
    P.lfq_region_set_summary.argtypes = [C.c_void_p, EMIT, C.c_void_p]
    P.lfq_region_begin.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int64]
    P.lfq_region_add_read.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_char_p, C.c_char_p]
    P.lfq_region_end.argtypes = [C.c_void_p]
    P.lfq_region_close.argtypes = [C.c_void_p, C.c_void_p]
    assert P.lfq_region_open(C.byref(h), caller.h, C.byref(conf.c), C.byref(o), cb_vcf, None) == 0
    if with_summary:
        assert P.lfq_region_set_summary(h, cb_sum, None) == 0
    n_cols = 0
    for k, (beg, end) in enumerate(regions):
        assert P.lfq_region_begin(h, b"chr1", genome, len(genome), beg, end) == 0
        if k == 1:
            assert P.lfq_region_set_summary(h, cb_sum, None) == -1         # not while a region is open or in flight
        for r in reads:
            rlen = sum(l for op, l in r["cigar"] if op in "MDN=X")
            if r["pos0"] >= end or r["pos0"] + rlen <= beg:
                continue
            seq4, cig, bi, bd = _bam_fields(r)
            q = np.asarray(r["qual"], np.uint8)
            assert P.lfq_region_add_read(h, r["pos0"], 16 if r["reverse"] else 0, r["mapq"], len(cig), cig.ctypes.data, len(q),
                                         seq4.ctypes.data, q.ctypes.data, bi, bd) == 1
        assert P.lfq_region_end(h) == 0
    assert P.lfq_region_close(h, None) == 0
    return out, n_cols


def test_three_regions_with_and_without_the_summary_callback(caller, tmp_path):
    import lofreq_amd as la
    from lofreq_amd import _lib
    lib = _build_region_lib(tmp_path)
    fx, reads = ref.load_golden("plpsummary_indel")
    genome = fx["genome"].encode()
    n = len(genome)
    regions = [(0, n // 3), (n // 3, n // 3 + 37), (n // 3 + 37, n)]
    L = _lib.load()
    st = _lib.SummaryTimes()

    conf0 = la.VarcallConf()
    # a summary call of another read set first, so that "no launch" below is this run's doing
    rs = la.ReadSet(caller, reads[:20], genome)
    rs.plp_summary(0, n)
    assert rs.last_summary_times().n_launches == 1
    rs.close()
    plain, _ = _run(caller, lib, reads, genome, regions, conf0, with_summary=False)
    assert L.lfq_last_summary_times(caller.h, C.byref(st)) == 0
    before = (st.n_launches, st.n_cols)
    assert all(tag == "V" for tag, _ in plain) and len(plain) > 5
    # without the callback the binding made no summary call: the context still reports the 20-read call above
    assert before == (1, rs_cols(reads[:20]))

    conf1 = la.VarcallConf()
    both, _ = _run(caller, lib, reads, genome, regions, conf1, with_summary=True)
    assert [s for tag, s in both if tag == "S"] == fx["lines"]
    assert [s for tag, s in both if tag == "V"] == [s for _, s in plain]
    assert (conf1.num_snv_tests, conf1.num_indel_tests, conf1.bonf_subst, conf1.bonf_indel) == \
        (conf0.num_snv_tests, conf0.num_indel_tests, conf0.bonf_subst, conf0.bonf_indel)
    assert conf1.num_indel_tests > 0 and conf1.num_snv_tests > 0
    # per region: its summary lines come before its VCF lines, regions in order
    pos = lambda tag, s: int(s.split("\t")[1]) - 1
    k = 0
    for beg, end in regions:
        seen_vcf = False
        while k < len(both) and beg <= pos(*both[k]) < end:
            if both[k][0] == "V":
                seen_vcf = True
            else:
                assert not seen_vcf, both[k]
            k += 1
    assert k == len(both)
    assert L.lfq_last_summary_times(caller.h, C.byref(st)) == 0 and st.n_launches == 1


def rs_cols(reads):
    """covered positions of a few reads"""
    s = set()
    for r in reads:
        x = r["pos0"]
        for op, l in r["cigar"]:
            if op in "MDN=X":
                s.update(range(x, x + l))
                x += l
    return len(s)
