"""-m gpu: `lofreq indelqual` on the device (lfq_indelqual_batch, lfq_readset_indelqual; lofreq_amd/csrc/lfq_indelqual.hip).

Bytes and integers only, no tolerance: the library gives the BI / BD strings the reference's 2.1.4 binary wrote for every
fixture read in every mode (tests/golden/indelqual_*.json), the strings of the plain-Python model (tests/indelqual_model.py,
itself held against the binary on the CPU) for a randomised batch, the same strings whatever the batch neighbours and however
the batch is cut; the read-set step feeds the indel pileup so that the reads -> VCF chain writes the lines of the binary's own
`indelqual --dindel` + `call --call-indels` run and, byte for byte, the records of the chain fed the same tags as host arrays;
the region binding with the option on equals the binding fed host tags."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import golden_reads as gr
import golden_util as gu
import indelqual_model as im
import indelqual_reads as ir
from test_indelqual_model import FAMILIES, GOLDEN, load_family, model_tags

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


def lib_reads(reads):
    """fixture reads -> the dicts lofreq_amd.indelqual_batch takes (bases and qualities are not read: zeros of the right length)"""
    out = []
    for r in reads:
        lq = r["l_qseq"] if "l_qseq" in r else len(r["seq"])
        out.append({"pos0": r["pos0"], "cigar": [tuple(c) for c in r["cigar"]], "seq": np.zeros(lq, np.uint8),
                    "qual": np.zeros(lq, np.uint8)})
    return out


def run_mode(la, caller, reads, genome, mode):
    """-> [(BI, BD)] as str"""
    if mode == "dindel":
        got = la.indelqual_batch(caller, reads, genome.encode(), "dindel")
    else:
        got = la.indelqual_batch(caller, reads, genome.encode(), "uniform", *ir.mode_quals(mode))
    return [(a.decode("latin-1"), b.decode("latin-1")) for a, b in got]


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("mode", ir.MODES)
def test_batch_gives_the_binarys_tags(caller, name, mode):
    import lofreq_amd as la
    fx, genome, reads = load_family(name)
    got = run_mode(la, caller, lib_reads(reads), genome, mode)
    assert len(got) == fx["n_reads"]
    for i, r in enumerate(reads):
        assert got[i] == ir.fixture_tags(fx["results"][mode], i), (name, mode, r["name"])


def test_batch_gives_the_models_tags_on_random_reads(caller):
    import lofreq_amd as la
    from lofreq_amd import indelqual as iq
    R = ir.make(seed=555, n=22000, glen=20000)
    reads = R["reads"]
    assert len(reads) >= 20000 and {len(r["seq"]) for r in reads} >= {36, 75, 150, 250, 340}
    lr = lib_reads(reads)
    for mode in ("dindel", "u17,3"):
        assert run_mode(la, caller, lr, R["genome"], mode) == model_tags(
            R["genome"], [dict(r, l_qseq=len(r["seq"])) for r in reads], mode), mode
    t = iq.last_times(caller)
    assert t["n_reads"] == len(reads) and t["n_bases"] == sum(len(r["seq"]) for r in reads)
    assert t["n_launches"] == 1 and t["ms_kernels"] > 0          # the uniform call: one fill


def test_neighbours_and_cuts_do_not_matter(caller):
    import lofreq_amd as la
    fx, genome, reads = load_family("indelqual_shapes")
    lr = lib_reads(reads)
    whole = run_mode(la, caller, lr, genome, "dindel")
    order = np.random.default_rng(3).permutation(len(lr))
    shuffled = run_mode(la, caller, [lr[i] for i in order], genome, "dindel")
    assert [shuffled[k] for k in np.argsort(order)] == whole
    cuts, at, sizes = [0], 0, [1, 7, 64, 1, 333, 2, 1000, 65]
    while at < len(lr):
        at = min(len(lr), at + sizes[len(cuts) % len(sizes)])
        cuts.append(at)
    pieces = []
    for a, b in zip(cuts, cuts[1:]):
        pieces += run_mode(la, caller, lr[a:b], genome, "dindel")
    assert pieces == whole


def test_empty_batch_and_refusals(caller):
    import lofreq_amd as la
    from lofreq_amd import _lib, indelqual as iq
    from lofreq_amd.viterbi import pack_reads
    ref = b"ACGTTTGACCA" * 30
    assert la.indelqual_batch(caller, [], ref, "dindel") == []
    assert iq.last_times(caller)["n_launches"] == 0
    ok = {"pos0": 5, "cigar": [("M", 20), ("I", 2), ("M", 8)], "seq": np.zeros(30, np.uint8), "qual": np.zeros(30, np.uint8)}
    assert len(la.indelqual_batch(caller, [ok], ref, "dindel")[0][0]) == 30

    def rc_of(reads, conf):
        rd, keep = pack_reads(reads, ref)
        out = np.zeros(4096, np.uint8)
        return _lib.load().lfq_indelqual_batch(caller.h, C.byref(rd), C.byref(conf), out.ctypes.data, out.ctypes.data)
    n_op = dict(ok, cigar=[("M", 20), ("N", 50), ("M", 10)])
    p_op = dict(ok, cigar=[("M", 20), ("P", 1), ("M", 10)])
    short = dict(ok, cigar=[("M", 29)])
    long_ = dict(ok, cigar=[("M", 20), ("S", 11)])
    neg = dict(ok, pos0=-1)
    for bad in (n_op, p_op, short, long_, neg):
        assert rc_of([ok, bad, ok], iq.make_conf("dindel")) == -1, bad          # LFQ_ERR_INVALID
    assert rc_of([ok], iq.make_conf(0)) == -1 and rc_of([ok], iq.make_conf(3)) == -1
    assert rc_of([ok, n_op], iq.make_conf("uniform", 40)) == 0                  # uniform mode looks at no CIGAR
    assert rc_of([ok], iq.make_conf("dindel")) == 0


def _chain(la, caller, R, kw, ndf, idq_mode):
    """the reads -> VCF chain of tests/test_gpu_big_golden.py with lfq_readset_indelqual between BAQ + IDAQ and the pileups
    -> (lines, conf, n_indel_tests, indel records, SNV records, fetched (bi, bd) or None)"""
    glen = R["glen"]
    rs = la.ReadSet.from_arrays(caller, R)
    rs.baq(extended=True, idaq=True)
    tags = None
    if idq_mode:
        rs.indelqual(idq_mode)
    conf = la.VarcallConf(**kw)
    lines = []
    cols, col_pos = rs.pileup_indels(0, glen)
    irecs, n_indel_tests = la.call_indels(caller, cols, conf)
    ikeep = la.filter_indel_records(irecs, la.snvqual_thresh(conf.sig, conf.bonf_indel), apply_defaults=not ndf)
    for r, k in zip(irecs, ikeep):
        if k:
            p0 = int(col_pos[int(r["col"])])
            lines.append((p0, 0, la.format_indel_record("chr1", p0, cols, r, "PASS").rstrip("\n")))
    dt = rs.pileup_snv(0, glen)
    la.skip_snv_columns(caller, cols.cons_indel)
    recs, _, _ = caller.call_snvs(dt, conf)
    keep = la.filter_records(recs, la.snvqual_thresh(conf.sig, conf.bonf_subst), apply_defaults=not ndf)
    for r, k in zip(recs, keep):
        if k:
            p0 = int(dt.col_pos[int(r["col"])])
            lines.append((p0, 1, la.format_vcf(np.array([r]), "chr1", pos0=np.array([p0]), filter_str="PASS").rstrip("\n")))
    if idq_mode:
        tags = rs.fetch_indelquals()
    rs.close()
    return [l[2] for l in sorted(lines, key=lambda t: (t[0], t[1]))], conf, n_indel_tests, irecs.copy(), recs.copy(), tags


def _model_arrays(R):
    """the model's BI (= BD) bytes of a golden_reads read set, in the seq_off layout"""
    table = im.dindel_table(R["ref"].decode())
    ops = "MIDNSHP=X"
    out = []
    for i in range(R["n"]):
        cig = [(ops[int(w) & 15], int(w) >> 4) for w in R["cig"][R["cig_off"][i]:R["cig_off"][i + 1]]]
        out.append(im.dindel_read(table, int(R["pos"][i]), cig))
    return np.frombuffer("".join(out).encode(), np.uint8).copy()


def test_readset_chain_writes_the_binarys_vcf(caller):
    import lofreq_amd as la
    fx = json.load(open(os.path.join(GOLDEN, "indelqual_e2e.json")))
    R = gr.make(**fx["generator"]["params"])
    R["bi"] = R["bd"] = None
    R["flags"] = np.zeros(R["n"], np.uint8)
    assert gr.sam_sha256(R) == fx["sam_sha256"]
    kw, ndf = gu.conf_kwargs(fx["call_args"])
    lines, conf, n_indel_tests, irecs, recs, tags = _chain(la, caller, R, kw, ndf, "dindel")
    # (a) the binary's own indelqual --dindel + call --call-indels
    assert conf.num_snv_tests == fx["num_tests"]["snv"] and n_indel_tests == fx["num_tests"]["indel"]
    assert [gu.strip_hqa(l) for l in lines] == fx["vcf"]
    # (b) the same chain fed the model's tags as host arrays: the same records, byte for byte
    model = _model_arrays(R)
    assert len(model) == int(R["seq_off"][-1])
    assert np.array_equal(tags[0], model) and np.array_equal(tags[1], model)
    H = dict(R, bi=model, bd=model.copy(), flags=np.full(R["n"], 3, np.uint8))
    lines_h, conf_h, n_h, irecs_h, recs_h, _ = _chain(la, caller, H, kw, ndf, None)
    assert lines_h == lines and n_h == n_indel_tests and conf_h.num_snv_tests == conf.num_snv_tests
    assert irecs_h.tobytes() == irecs.tobytes() and recs_h.tobytes() == recs.tobytes()
    assert len(irecs) >= 20
    # the step supersedes arrays the caller did upload ("Both will overwrite any existing values")
    W = dict(R, bi=np.full(len(model), 33 + 7, np.uint8), bd=np.full(len(model), 33 + 7, np.uint8), flags=np.full(R["n"], 3, np.uint8))
    lines_w, _, _, irecs_w, _, tags_w = _chain(la, caller, W, kw, ndf, "dindel")
    assert lines_w == lines and irecs_w.tobytes() == irecs.tobytes() and np.array_equal(tags_w[0], model)


def test_readset_uniform_equals_host_arrays(caller):
    import lofreq_amd as la
    fx = json.load(open(os.path.join(GOLDEN, "indelqual_e2e.json")))
    R = gr.make(**fx["generator"]["params"])
    R["bi"] = R["bd"] = None
    R["flags"] = np.zeros(R["n"], np.uint8)
    kw, ndf = gu.conf_kwargs(fx["call_args"])
    rs_lines = None
    for idq in (True, False):
        nb = int(R["seq_off"][-1])
        P = R if idq else dict(R, bi=np.full(nb, 33 + 40, np.uint8), bd=np.full(nb, 33 + 40, np.uint8), flags=np.full(R["n"], 3, np.uint8))
        rs = la.ReadSet.from_arrays(caller, P)
        rs.baq(extended=True, idaq=True)
        if idq:
            rs.indelqual("uniform", 40)
            bi, bd = rs.fetch_indelquals()
            assert (bi == 33 + 40).all() and (bd == 33 + 40).all() and len(bi) == nb
        conf = la.VarcallConf(**kw)
        cols, col_pos = rs.pileup_indels(0, R["glen"])
        irecs, n_tests = la.call_indels(caller, cols, conf)
        ikeep = la.filter_indel_records(irecs, la.snvqual_thresh(conf.sig, conf.bonf_indel), apply_defaults=not ndf)
        lines = [la.format_indel_record("chr1", int(col_pos[int(r["col"])]), cols, r, "PASS").rstrip("\n")
                 for r, k in zip(irecs, ikeep) if k]
        rs.close()
        if idq:
            rs_lines = (lines, n_tests, irecs.tobytes())
        else:
            assert (lines, n_tests, irecs.tobytes()) == rs_lines
    # ... and they are the lines the binary wrote after `indelqual -u 40`
    assert rs_lines[0] == fx["indel_lines_after_uniform_40"]


def _run_binding(caller, lib, reads, ref, regions, conf, idq_conf):
    """tests/test_gpu_chain.py::_run_regions with lfq_region_set_indelqual"""
    from test_gpu_chain import _RegionOpts, _bam_fields
    P = C.CDLL(lib)
    lines = []
    EMIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)
    cb = EMIT(lambda user, s: lines.append(s.decode().rstrip("\n")))
    o = _RegionOpts()
    P.lfq_region_opts_init(C.byref(o))
    o.use_idaq, o.call_indels = 1, 1
    h = C.c_void_p()
    P.lfq_region_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, EMIT, C.c_void_p]
    assert P.lfq_region_open(C.byref(h), caller.h, C.byref(conf.c), C.byref(o), cb, None) == 0
    P.lfq_region_set_indelqual.argtypes = [C.c_void_p, C.c_void_p]
    if idq_conf is not None:
        assert P.lfq_region_set_indelqual(h, C.byref(idq_conf)) == 0
    P.lfq_region_begin.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int64]
    P.lfq_region_add_read.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_char_p, C.c_char_p]
    P.lfq_region_end.argtypes = [C.c_void_p]
    P.lfq_region_close.argtypes = [C.c_void_p, C.c_void_p]
    for beg, end in regions:
        assert P.lfq_region_begin(h, b"chr1", ref, len(ref), beg, end) == 0
        for r in reads:
            rlen = sum(l for op, l in r["cigar"] if op in "MDN=X")
            if r["pos0"] >= end or r["pos0"] + rlen <= beg:
                continue
            seq4, cig, bi, bd = _bam_fields(r)
            q = np.asarray(r["qual"], np.uint8)
            assert P.lfq_region_add_read(h, r["pos0"], 16 if r["reverse"] else 0, r["mapq"], len(cig), cig.ctypes.data, len(q),
                                         seq4.ctypes.data, q.ctypes.data, bi, bd) in (0, 1)
        assert P.lfq_region_end(h) == 0
    wo = C.c_int64(-1)
    assert P.lfq_region_close(h, C.byref(wo)) == 0
    return lines


@pytest.mark.parametrize("mode", ["dindel", "u40,25"])
def test_region_binding_with_the_option_equals_host_tags(caller, tmp_path, mode):
    import lofreq_amd as la
    from lofreq_amd import indelqual as iq
    from test_gpu_chain import _build_region_lib
    lib = _build_region_lib(tmp_path)
    fx, reads = gu.load_plpindel(gu.plpindel_fixtures()[-1], with_alnqual_tags=False)
    genome = fx["genome"]
    ref = genome.encode()
    kw, _ = gu.conf_kwargs(fx["call_args"])
    tags = model_tags(genome, [dict(r, l_qseq=len(r["seq"])) for r in reads], mode)
    bare = [dict(r, bi=None, bd=None) for r in reads]
    tagged = [dict(r, bi=np.frombuffer(t[0].encode(), np.uint8), bd=np.frombuffer(t[1].encode(), np.uint8)) for r, t in zip(reads, tags)]
    idq = iq.make_conf("dindel") if mode == "dindel" else iq.make_conf("uniform", *ir.mode_quals(mode))
    n = len(ref)
    for regions in ([(0, n)], [(0, n // 3), (n // 3, n // 3 + 37), (n // 3 + 37, n)]):
        c_on, c_host, c_off = la.VarcallConf(**kw), la.VarcallConf(**kw), la.VarcallConf(**kw)
        on = _run_binding(caller, lib, bare, ref, regions, c_on, idq)
        host = _run_binding(caller, lib, tagged, ref, regions, c_host, None)
        assert on == host and any("INDEL" in l for l in on)
        assert (c_on.num_snv_tests, c_on.num_indel_tests, c_on.bonf_indel) == (c_host.num_snv_tests, c_host.num_indel_tests, c_host.bonf_indel)
        # default off: reads without tags stay without (quality 0: the binding as it was)
        off = _run_binding(caller, lib, bare, ref, regions, c_off, None)
        assert off != on
