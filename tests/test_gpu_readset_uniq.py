"""-m gpu: `lofreq uniq` on the reads of a resident read set -- lfq_readset_pileup_sites (the sparse pileup: column i = site i)
and lfq_readset_uniq (uniq_snv for SNV and indel variants, both modes) -- against the oracle road on every row of the case
table (tests/uniq_sites_cases.py; tests/test_uniq_sites_cases.py holds that road against plain restatements and the binary
without a GPU), against the values the 2.1.4 binary stored (uniq_reads.json, uniq_detlim.json), and its refusals."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import golden_util as gu
import uniq_sites_cases as uc
import util

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


def _fetch(ptr, nbytes):
    """device memory at a raw pointer -> numpy"""
    hip = C.CDLL("libamdhip64.so")
    out = np.zeros(max(nbytes, 1), np.uint8)
    if nbytes:
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0   # DeviceToHost
    return out[:nbytes]


def _columns(t):
    """the device tracks `t` (unpacked nt) on the host"""
    n = int(t.ncols)
    off = _fetch(t.col_off, (n + 1) * 8).view(np.uint64)
    n_obs = int(off[-1])
    return dict(col_off=off, nt=_fetch(t.nt, n_obs), bq=_fetch(t.bq, n_obs), baq=_fetch(t.baq, n_obs), mq=_fetch(t.mq, n_obs),
                ref_base=_fetch(t.ref_base, n), cov=_fetch(t.coverage_plp, n * 4).view(np.int32),
                nb=_fetch(t.num_bases, n * 4).view(np.int32))


def _uniq(rs, var, af=None, **kw):
    return rs.uniq([v[0] for v in var], [v[1] for v in var], [v[2] for v in var],
                   [(v[3] if af is None else af) for v in var], [v[4] for v in var], **kw)


@pytest.mark.parametrize("case", uc.cases(), ids=uc.case_ids())
def test_case_table_against_the_oracle_road(caller, oracle, case):
    import lofreq_amd as la
    reads, ref, var, min_bq = case["reads"], case["ref"], case["variants"], case["min_plp_bq"]
    pos = [v[0] for v in var]
    n = len(var)
    S = uc.oracle_sites(oracle, reads, ref, pos, min_bq)
    U = uc.oracle_uniq(oracle, S, var)
    rs = la.ReadSet(caller, reads, ref.encode())
    try:
        dt, cov, tails = rs.pileup_sites(pos, min_bq)
        t = dt._tracks()
        G = _columns(t)
        assert t.ncols == n and t.flags == 0 and t.max_col_obs == (int(S["nb"].max()) if n else 0) and not t.sq
        assert G["col_off"].tolist() == S["col_off"].tolist()
        for k in ("nt", "bq", "mq", "ref_base", "cov", "nb"):                   # byte for byte, in pileup order
            assert np.array_equal(G[k], S[k]), k
        assert (G["baq"] == 255).all()                                          # no BAQ in this read set
        assert cov.tolist() == S["cov"].tolist() and tails.tolist() == S["tails"].tolist()
        ts = rs.last_sites_times()
        assert ts.n_sites == n and ts.n_obs == int(S["col_off"][-1]) and ts.n_launches == (2 if ts.n_obs else 1)
        assert ts.count_ms > 0 and (ts.scatter_ms > 0) == (ts.n_obs > 0)
        # the det-lim p-values on these very tracks
        af = np.asarray([v[3] for v in var], np.float32)
        det, pv = caller.uniq_detlim(dt, af)
        assert det.tolist() == U["detlim_flag"].tolist()
        for i in np.flatnonzero(det):
            util.assert_pvalue_close(pv[i], U["detlim_pvalue"][i], ctx="%s site %d" % (case["name"], i))
        # the same columns as the region pileup hands out at these positions
        caller.set_pileup_nt_packed(False)
        try:
            reg = rs.pileup_snv(0, len(ref), min_bq, sync=True)
        finally:
            caller.set_pileup_nt_packed(True)
        R = _columns(reg._tracks())
        col_of = {int(p): i for i, p in enumerate(reg.col_pos)}
        for i, p in enumerate(pos):
            ci = col_of.get(p)
            a, b = int(G["col_off"][i]), int(G["col_off"][i + 1])
            if ci is None:
                assert a == b and G["cov"][i] == 0
                continue
            c, d = int(R["col_off"][ci]), int(R["col_off"][ci + 1])
            for k in ("nt", "bq", "baq", "mq"):
                assert np.array_equal(G[k][a:b], R[k][c:d]), (k, p)
            assert (G["ref_base"][i], G["cov"][i], G["nb"][i]) == (R["ref_base"][ci], R["cov"][ci], R["nb"][ci])
        # uniq_snv, both modes
        r = _uniq(rs, var, min_plp_bq=min_bq)
        for k in ("coverage", "alt_count", "uq"):
            assert r[k].tolist() == U[k].tolist(), k
        ok = U["uq"] >= 0
        assert (r["pvalue"][~ok] == -1.0).all() and np.allclose(r["pvalue"][ok], U["pvalue"][ok], rtol=1e-11, atol=1e-300)
        assert not r["detectable"].any()
        for mtc in ("fdr", "holm"):
            assert la.uniq_mtc(r["uq"], mtc, 0.001, 0).tolist() == oracle.uniq_mtc(U["uq"], mtc, 0.001, 0).tolist()
        r = _uniq(rs, var, use_det_lim=True, min_plp_bq=min_bq)
        assert r["detectable"].tolist() == U["detectable"].tolist() and r["coverage"].tolist() == U["coverage"].tolist()
        assert (r["uq"] == -1).all() and (r["pvalue"] == -1.0).all() and not r["alt_count"].any()
    finally:
        rs.close()


@pytest.mark.parametrize("run", ["default", "detlim", "unifreq"])
def test_uniq_reads_equal_the_reference_binary(caller, run):
    """uniq_reads.json: the stored reads, filtered HERE as uniq's mpileup filters them, against the UQ= values, UNIQ flags and
    FILTER columns of the three runs of the 2.1.4 binary"""
    import lofreq_amd as la
    fx, ref, reads, var = uc.load_uniq_reads()
    uq, flags, passed = uc.binary_run(fx, run)
    rs = la.ReadSet(caller, reads, ref.encode())
    try:
        r = _uniq(rs, var, af=0.5 if run == "unifreq" else None, use_det_lim=run == "detlim")
    finally:
        rs.close()
    if run == "detlim":
        assert r["detectable"].astype(bool).tolist() == flags
    else:
        assert r["uq"].tolist() == uq and not r["detectable"].any()
        assert la.uniq_mtc(r["uq"], fx["mtc"], fx["alpha"], 0).tolist() == passed


def test_uniq_detlim_fixture_from_regenerated_reads(caller):
    """uniq_detlim.json stores columns, not reads: the reads are regenerated with the fixture's generator call, shown to give
    the stored per-nucleotide counts at every variant under uniq's filter, and then taken through lfq_readset_uniq"""
    import lofreq_amd as la
    import make_golden as mg
    path = [p for p in gu.uniq_fixtures() if p.endswith("uniq_detlim.json")][0]
    fx, _, af = gu.load_uniq(path)
    with tempfile.TemporaryDirectory() as tmp:
        ref = mg.write_fixture(tmp, 81, 400, 700, {}, [60] * 24 + [40, 30, 20, 10, 0, 255])
        reads = []
        for line in open(os.path.join(tmp, "t.sam")):
            if line.startswith("@"):
                continue
            f = line.rstrip("\n").split("\t")
            if uc.uniq_filter(int(f[1]), int(f[4])):
                reads.append({"pos0": int(f[3]) - 1, "cigar": uc.parse_cigar(f[5]), "mapq": int(f[4]), "reverse": bool(int(f[1]) & 16),
                              "seq": np.asarray([uc.CODE.get(c, 4) for c in f[9]], np.uint8),
                              "qual": np.asarray([ord(c) - 33 for c in f[10]], np.uint8)})
    plain = gu.py_pileup(reads, 3)
    V = fx["variants"]
    assert len(V) == 130
    for v in V:
        col = plain.get(v["pos0"], {})
        assert {nt: len(x) for nt, x in col.items()} == {nt: len(gu.dec(o["bq"])) for nt, o in v["obs"].items() if o["bq"]}, v["pos0"]
        assert v["ref"] == ref[v["pos0"]]
    rs = la.ReadSet(caller, reads, ref.encode())
    try:
        r = rs.uniq([v["pos0"] for v in V], [v["ref"] for v in V], [v["alt"] for v in V], af, use_det_lim=True)
    finally:
        rs.close()
    assert r["detectable"].astype(bool).tolist() == [v["uniq"] for v in V]


def test_refusals_trivial_cases_and_the_region_tracks_stay(caller):
    import lofreq_amd as la
    from lofreq_amd import _lib, pileup
    L = _lib.load()
    ref, reads = uc._mixed_reads()
    rs = la.ReadSet(caller, reads, ref.encode())
    try:
        # the tracks of the region pileup are other buffers: unchanged by a sites call, and still what skip_snv_columns edits
        reg = rs.pileup_snv(100, 300, sync=True)
        before = {k: v.copy() for k, v in _columns_packed(reg._tracks()).items()}
        dt, cov, tails = rs.pileup_sites([150, 20, 150, 699])
        assert cov[0] == cov[2] > 0
        after = _columns_packed(reg._tracks())
        assert all(np.array_equal(before[k], after[k]) for k in before)
        pileup.skip_snv_columns(caller, np.zeros(reg.ncols, np.uint8))
        # n = 0: nothing is launched
        dt0, cov0, _ = rs.pileup_sites([])
        assert dt0.ncols == 0 and len(cov0) == 0 and rs.last_sites_times().n_launches == 0
        assert all(len(v) == 0 for v in rs.uniq([], [], [], []).values()) and rs.last_sites_times().n_launches == 0
        # refusals, each LFQ_ERR_INVALID
        for bad in ([-1], [len(ref)], [5, 1 << 40]):
            with pytest.raises(RuntimeError, match=r"\(-1\)"):
                rs.pileup_sites(bad)
        t = _lib.Tracks()
        one = np.asarray([5], np.int64)
        assert L.lfq_readset_pileup_sites(caller.h, rs.h, one.ctypes.data, -1, 3, C.byref(t), None, None) == -1
        assert L.lfq_readset_pileup_sites(caller.h, rs.h, None, 1, 3, C.byref(t), None, None) == -1
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            rs.uniq([5], ["A"], ["C"], [float("nan")])
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            rs.uniq([700], ["A"], ["C"], [0.1])
        v, o = _lib.UniqVariants(), _lib.UniqResult()
        v.n = -1
        assert L.lfq_readset_uniq(caller.h, rs.h, C.byref(v), 0, 3, C.byref(o)) == -1
        off_bad, off_ok = np.asarray([1, 0], np.int64), np.asarray([0, 1], np.int64)
        af = np.asarray([0.1], np.float32)
        for ro, ao in ((off_bad, off_ok), (off_ok, off_bad)):
            v = _lib.UniqVariants()
            v.n, v.pos, v.ref_off, v.alt_off, v.af = 1, one.ctypes.data, ro.ctypes.data, ao.ctypes.data, af.ctypes.data
            v.ref = v.alt = C.cast(C.c_char_p(b"AC"), C.c_void_p)
            assert L.lfq_readset_uniq(caller.h, rs.h, C.byref(v), 0, 3, C.byref(o)) == -1
        # a -d cap that drops a read of the region is refused; one that drops none is not
        assert rs.kept_reads(max_depth=1)[1] < len(reads)
        with pileup._MaxDepth(caller, 1):
            with pytest.raises(RuntimeError, match=r"\(-1\)"):
                rs.pileup_sites([150])
            with pytest.raises(RuntimeError, match=r"\(-1\)"):
                rs.uniq([150], ["A"], ["C"], [0.1])
        with pileup._MaxDepth(caller, 100000):
            assert rs.pileup_sites([150])[1][0] == cov[0]
    finally:
        rs.close()
    # reads that are not position-sorted, also after lfq_set_pileup_unsorted
    rs = la.ReadSet(caller, reads[::-1], ref.encode())
    try:
        for on in (False, True):
            caller.set_pileup_unsorted(on)
            with pytest.raises(RuntimeError, match=r"\(-1\)"):
                rs.pileup_sites([150])
    finally:
        caller.set_pileup_unsorted(False)
        rs.close()


def _columns_packed(t):
    """every byte of region tracks (packed nt) a later call could have overwritten"""
    n = int(t.ncols)
    off = _fetch(t.col_off, (n + 1) * 8).view(np.uint64)
    n_obs = int(off[-1])
    return dict(col_off=off, nt=_fetch(t.nt, (n_obs + 7) // 8 * 4), bq=_fetch(t.bq, n_obs), baq=_fetch(t.baq, n_obs),
                mq=_fetch(t.mq, n_obs), ref_base=_fetch(t.ref_base, n), cov=_fetch(t.coverage_plp, n * 4), nb=_fetch(t.num_bases, n * 4))
