"""-m gpu: -d / --max-depth on the read-level path (lfq_set_max_depth, lfq_readset_kept_reads, lfq_region_set_max_depth)
against the rule restated in tests/maxdepth_model.py and the reference's 2.1.4 binary (tests/golden/maxdepth_*.json)."""
import ctypes as C
import os

import numpy as np
import pytest

import maxdepth_model as mm

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

LFQ_ERR_INVALID = -1


def _fetch(ptr, nbytes):
    hip = C.CDLL("libamdhip64.so")
    out = np.zeros(max(nbytes, 1), np.uint8)
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0
    return out[:nbytes]


def _tracks_host(caller, dt):
    """every byte of device tracks (one nt byte per observation: the caller runs with set_pileup_nt_packed(False))"""
    caller.synchronize()
    t = dt._tracks()
    n = dt.ncols
    off = _fetch(t.col_off, (n + 1) * 8).view(np.uint64)
    n_obs = int(off[-1])
    out = {"col_pos": np.asarray(dt.col_pos), "col_off": off, "max_col_obs": dt.max_col_obs,
           "ref_base": _fetch(t.ref_base, n), "cov": _fetch(t.coverage_plp, n * 4).view(np.int32),
           "nb": _fetch(t.num_bases, n * 4).view(np.int32)}
    for k in ("nt", "bq", "baq", "mq"):
        out[k] = _fetch(getattr(t, k), n_obs)
    return out


def _assert_tracks_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def _indel_summary(cols, col_pos):
    from lofreq_amd.indel import _I32
    d = {"col_pos": np.asarray(col_pos), "cons": np.asarray(cols.cons_indel), "keys": cols.keys}
    for n in _I32:
        d[n] = np.asarray(getattr(cols, n))
    for sd in (0, 1):
        for k, v in (cols.sides[sd] or {}).items():
            if v is not None:
                d["%d_%s" % (sd, k)] = np.asarray(v)
    return d


def _assert_summary_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "keys":
            assert a[k] == b[k]
        else:
            assert np.array_equal(a[k], b[k]), k


def _random_reads(rng, glen, n, indels=True):
    """position-sorted reads with runs of equal starts, unequal spans, S / I / D / N, both strands, BI / BD"""
    starts = np.sort(np.concatenate([rng.integers(0, glen - 300, n), np.repeat(rng.integers(0, glen - 300, n // 40), 30)]))
    reads = []
    for pos in starts.tolist():
        body = int(rng.integers(15, 160))
        k = int(rng.integers(0, 6)) if indels else 5
        cigar = [("S", int(rng.integers(1, 8)))] if rng.random() < 0.2 else []
        if k == 0:
            cigar += [("M", int(rng.integers(5, 40))), ("I", int(rng.integers(1, 5))), ("M", body)]
        elif k == 1:
            cigar += [("M", int(rng.integers(5, 40))), ("D", int(rng.integers(1, 6))), ("M", body)]
        elif k == 2:
            cigar += [("M", int(rng.integers(5, 40))), ("N", int(rng.integers(5, 120))), ("M", body)]
        else:
            cigar += [("M", body)]
        ql = sum(l for o, l in cigar if o in "MIS=X")
        reads.append({"pos0": int(pos), "cigar": cigar, "seq": rng.integers(0, 5, ql).astype(np.uint8),
                      "qual": rng.integers(0, 45, ql).astype(np.uint8), "mapq": int(rng.integers(0, 61)),
                      "reverse": bool(rng.integers(0, 2)), "lb": rng.integers(33, 100, ql).astype(np.uint8),
                      "bi": rng.integers(33, 80, ql).astype(np.uint8), "bd": rng.integers(33, 80, ql).astype(np.uint8)})
    return reads


def _need(reads):
    """the smallest cap under which the model keeps every read"""
    pos = [r["pos0"] for r in reads]
    ends = [mm.ref_end(r["pos0"], r["cigar"]) for r in reads]
    lo, hi = 0, len(reads) + 1
    while lo < hi:
        mid = (lo + hi) // 2
        if mm.kept(pos, ends, mid).all():
            hi = mid
        else:
            lo = mid + 1
    return lo


def test_kept_reads_equal_the_model_on_the_fixtures(caller):
    import lofreq_amd as la
    for name in ("maxdepth_stacks", "maxdepth_chain"):
        fx, reads = mm.load(name)
        rs = la.ReadSet(caller, reads, fx["genome"].encode())
        try:
            for d in sorted({r["max_depth"] for r in fx["runs"]} | {0}):
                keep, n_kept = rs.kept_reads(d)
                want = mm.kept_reads(reads, d)
                assert np.array_equal(keep, want), (name, d)
                assert n_kept == int(want.sum())
            keep, n_kept = rs.kept_reads(None)
            assert keep.all() and n_kept == len(reads)
        finally:
            rs.close()


@pytest.mark.parametrize("seed,n", [(1, 3000), (2, 12000), (3, 260000)])
def test_kept_reads_equal_the_model_on_random_sets(caller, seed, n):
    """caps 0, 1, 2, need - 1, need, need + 1; the largest set is split over the host threads"""
    import lofreq_amd as la
    rng = np.random.default_rng(seed)
    glen = max(4000, n // 4)
    pos = np.sort(np.concatenate([rng.integers(0, glen, n - n // 10), np.repeat(rng.integers(0, glen, n // 300), 30)]))
    span = rng.integers(1, 200, len(pos))
    R = {"n": len(pos), "pos": pos.astype(np.int32), "cig_off": np.arange(len(pos) + 1, dtype=np.int64),
         "cig": (span.astype(np.uint32) << 4), "seq_off": np.cumsum(np.concatenate([[0], span])).astype(np.int64),
         "ref": b"A" * (glen + 400)}
    nb = int(R["seq_off"][-1])
    R["seq"], R["qual"] = np.zeros(nb, np.uint8), np.full(nb, 30, np.uint8)
    R["mapq"], R["rev"] = np.full(len(pos), 60, np.uint8), np.zeros(len(pos), np.uint8)
    ends = pos + span
    rs = la.ReadSet.from_arrays(caller, R)
    try:
        lo, hi = 0, 1 << 20
        while lo < hi:                                   # smallest cap under which the model keeps every read
            mid = (lo + hi) // 2
            if mm.kept(pos, ends, mid).all():
                hi = mid
            else:
                lo = mid + 1
        need = lo
        assert need > 3
        for d in (0, 1, 2, need - 1, need, need + 1):
            keep, n_kept = rs.kept_reads(d)
            want = mm.kept(pos, ends, d)
            assert np.array_equal(keep, want), d
            assert n_kept == int(want.sum())
    finally:
        rs.close()


def test_pileups_under_the_cap_equal_plpsummary(caller):
    import lofreq_amd as la
    fx, reads = mm.load("maxdepth_stacks")
    ref = fx["genome"].encode()
    rs = la.ReadSet(caller, reads, ref)
    caller.set_pileup_nt_packed(False)
    try:
        rs.baq(idaq=True)
        for run in fx["runs"]:
            d = run["max_depth"]
            h = _tracks_host(caller, rs.pileup_snv(0, len(ref), max_depth=d))
            got = {}
            for c, p in enumerate(h["col_pos"]):
                a, b = int(h["col_off"][c]), int(h["col_off"][c + 1])
                for code in h["nt"][a:b]:
                    fr = got.setdefault(int(p), {}).setdefault("ACGTN"[min(code & 7, 4)], [0, 0])
                    fr[1 if code & 8 else 0] += 1
            assert got == mm.plpsummary_columns(run), d
            assert [int(p) for p in h["col_pos"]] == [c["pos0"] for c in run["columns"]], d
            cols, col_pos = rs.pileup_indels(0, len(ref), max_depth=d)
            assert np.array_equal(np.asarray(col_pos), h["col_pos"]), d           # the two pileups agree on the columns
            assert np.array_equal(np.asarray(cols.coverage_plp), h["cov"]), d
    finally:
        caller.set_pileup_nt_packed(True)
        rs.close()


@pytest.mark.parametrize("seed,n", [(11, 4000), (12, 30000)])
def test_capped_pileups_equal_uncapped_pileups_of_the_kept_reads(caller, seed, n):
    """every track byte and every indel field under the cap = the uncapped pileups of a read set holding the kept reads only;
    a cap at the need (nothing dropped) = no cap, byte for byte"""
    import lofreq_amd as la
    rng = np.random.default_rng(seed)
    glen = 6000
    reads = _random_reads(rng, glen, n)
    reads = [r for r in reads if mm.ref_end(r["pos0"], r["cigar"]) <= glen]
    ref = "".join(rng.choice(list("ACGT"), glen)).encode()
    need = _need(reads)
    caller.set_pileup_nt_packed(False)
    rs = la.ReadSet(caller, reads, ref)
    try:
        base = _tracks_host(caller, rs.pileup_snv(0, glen))
        base_i = _indel_summary(*rs.pileup_indels(0, glen))
        _assert_tracks_equal(_tracks_host(caller, rs.pileup_snv(0, glen, max_depth=need)), base)
        _assert_summary_equal(_indel_summary(*rs.pileup_indels(0, glen, max_depth=need)), base_i)
        for d in (need // 8, need // 2, need - 1):
            keep = mm.kept_reads(reads, d)
            assert 0 < keep.sum() < len(reads)
            sub = la.ReadSet(caller, [r for r, k in zip(reads, keep) if k], ref)
            try:
                want = _tracks_host(caller, sub.pileup_snv(0, glen))
                want_i = _indel_summary(*sub.pileup_indels(0, glen))
            finally:
                sub.close()
            _assert_tracks_equal(_tracks_host(caller, rs.pileup_snv(0, glen, max_depth=d)), want)
            _assert_summary_equal(_indel_summary(*rs.pileup_indels(0, glen, max_depth=d)), want_i)
            # and in the other order: indels first (the decision and the device list are shared)
            rs2 = la.ReadSet(caller, reads, ref)
            try:
                _assert_summary_equal(_indel_summary(*rs2.pileup_indels(0, glen, max_depth=d)), want_i)
                _assert_tracks_equal(_tracks_host(caller, rs2.pileup_snv(0, glen, max_depth=d)), want)
            finally:
                rs2.close()
        # the host-buffer wrappers take the cap too
        d = need // 2
        keep = mm.kept_reads(reads, d)
        kr = [r for r, k in zip(reads, keep) if k]
        lb_all = [r["lb"] for r in reads]
        _assert_tracks_equal(_tracks_host(caller, la.pileup_snv_tracks(caller, reads, ref, 0, glen, lb=lb_all, max_depth=d)),
                             _tracks_host(caller, la.pileup_snv_tracks(caller, kr, ref, 0, glen, lb=[r["lb"] for r in kr])))
        _assert_summary_equal(_indel_summary(*la.pileup_indel_columns(caller, reads, ref, 0, glen, max_depth=d)),
                              _indel_summary(*la.pileup_indel_columns(caller, kr, ref, 0, glen)))
    finally:
        caller.set_pileup_nt_packed(True)
        rs.close()


def test_unsorted_reads_with_a_cap_are_refused(caller):
    import lofreq_amd as la
    rng = np.random.default_rng(4)
    reads = _random_reads(rng, 2000, 300, indels=False)
    reads[10], reads[200] = reads[200], reads[10]
    ref = b"ACGT" * 600
    L = la._lib.load()
    caller.set_pileup_unsorted(True)
    rs = la.ReadSet(caller, reads, ref)
    try:
        rs.pileup_snv(0, 2000)                                   # without a cap the unsorted kernels take them
        assert L.lfq_set_max_depth(caller.h, 5) == 0
        n = C.c_int64(0)
        assert L.lfq_readset_kept_reads(caller.h, rs.h, None, C.byref(n)) == LFQ_ERR_INVALID
        t = la._lib.Tracks()
        col_pos = np.zeros(2000, np.int64)
        assert L.lfq_readset_pileup_snv(caller.h, rs.h, 0, 2000, 3, C.byref(t), col_pos.ctypes.data) == LFQ_ERR_INVALID
        out = C.POINTER(la._lib.IndelColumnsC)()
        assert L.lfq_readset_pileup_indels(caller.h, rs.h, 0, 2000, 0, C.byref(out), col_pos.ctypes.data) == LFQ_ERR_INVALID
        assert L.lfq_set_max_depth(caller.h, -2) == LFQ_ERR_INVALID
    finally:
        L.lfq_set_max_depth(caller.h, -1)
        caller.set_pileup_unsorted(False)
        rs.close()


# ---- the region binding -------------------------------------------------------------------------------------------------

def _region_run(caller, lib, reads, ref, conf, max_depth, call_indels=False):
    """one region over the whole contig through integration/lofreq_amd_region.c, with lfq_region_set_max_depth"""
    import test_gpu_chain as tc
    P = C.CDLL(lib)
    lines = []
    EMIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)
    cb = EMIT(lambda user, s: lines.append(s.decode().rstrip("\n")))
    o = tc._RegionOpts()
    P.lfq_region_opts_init(C.byref(o))
    o.use_idaq = o.call_indels = 1 if call_indels else 0
    h = C.c_void_p()
    P.lfq_region_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, EMIT, C.c_void_p]
    assert P.lfq_region_open(C.byref(h), caller.h, C.byref(conf.c), C.byref(o), cb, None) == 0
    P.lfq_region_set_max_depth.argtypes = [C.c_void_p, C.c_int64]
    if max_depth is not None:
        assert P.lfq_region_set_max_depth(h, max_depth) == 0
    P.lfq_region_begin.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int64]
    P.lfq_region_add_read.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_char_p, C.c_char_p]
    P.lfq_region_end.argtypes = [C.c_void_p]
    P.lfq_region_close.argtypes = [C.c_void_p, C.c_void_p]
    assert P.lfq_region_begin(h, b"chr1", ref, len(ref), 0, len(ref)) == 0
    for r in reads:
        seq4, cig, bi, bd = tc._bam_fields(r)
        q = np.asarray(r["qual"], np.uint8)
        assert P.lfq_region_add_read(h, r["pos0"], 16 if r["reverse"] else 0, r["mapq"], len(cig), cig.ctypes.data, len(q),
                                     seq4.ctypes.data, q.ctypes.data, bi, bd) in (0, 1)
    assert P.lfq_region_end(h) == 0
    wo = C.c_int64(-1)
    assert P.lfq_region_close(h, C.byref(wo)) == 0
    return lines


@pytest.mark.parametrize("name", ["maxdepth_stacks", "maxdepth_chain"])
def test_region_binding_writes_the_binary_vcf_under_the_cap(caller, tmp_path, name):
    import golden_util as gu
    import lofreq_amd as la
    import test_gpu_chain as tc
    lib = tc._build_region_lib(tmp_path)
    fx, reads = mm.load(name)
    ref = fx["genome"].encode()
    for run in fx["runs"]:
        kw, ndf = gu.conf_kwargs(run["call_args"])
        conf = la.VarcallConf(**kw)
        lines = _region_run(caller, lib, reads, ref, conf, run["max_depth"])
        assert conf.num_snv_tests == run["num_snv_tests"], run["max_depth"]
        got = tc._epilogue(la, lines, conf)
        if not ndf:
            got = [l for l in got if l in set(run["vcf"])]
        assert got == run["vcf"], (run["max_depth"], run["call_args"])
    # no setter call: the uncapped output, which for these reads is the 1 000 000 default's
    for run in [r for r in fx["runs"] if r["max_depth"] == 1000000]:
        kw, ndf = gu.conf_kwargs(run["call_args"])
        conf = la.VarcallConf(**kw)
        got = tc._epilogue(la, _region_run(caller, lib, reads, ref, conf, None), conf)
        if not ndf:
            got = [l for l in got if l in set(run["vcf"])]
        assert got == run["vcf"] and conf.num_snv_tests == run["num_snv_tests"]


@pytest.mark.parametrize("name", ["maxdepth_indel", "maxdepth_c4"])
def test_region_binding_with_indels_writes_the_binary_vcf_under_the_cap(caller, tmp_path, name):
    """BI / BD tags, `lofreq call --call-indels -d N`: SNV and indel lines and both test counts, byte for byte (the C4 shape:
    24 kb x 500x at -d 200, where the cap drops reads in every bin and the compaction spans many tiles)"""
    import golden_util as gu
    import lofreq_amd as la
    import test_gpu_chain as tc
    lib = tc._build_region_lib(tmp_path)
    fx, R = mm.load_generated(name)
    keep = mm.kept_flat(R, fx["max_depth"])
    assert 0 < keep.sum() < R["n"]
    kw, ndf = gu.conf_kwargs(fx["call_args"])
    conf = la.VarcallConf(**kw)
    lines = _region_run(caller, lib, mm.read_dicts(R), R["ref"], conf, fx["max_depth"], call_indels=True)
    assert conf.num_snv_tests == fx["num_tests"]["snv"] and conf.num_indel_tests == fx["num_tests"]["indel"]
    got = tc._epilogue(la, lines, conf)
    if not ndf:                                             # the default filter is `lofreq filter`'s business
        got = [l for l in got if l in set(fx["vcf"])]
    assert got == fx["vcf"]
    assert any("INDEL" in l for l in got)
