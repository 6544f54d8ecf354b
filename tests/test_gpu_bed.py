"""-m gpu: `lofreq call -l` on the read-level road (lfq_set_bed, lfq_region_set_bed) against tests/bed_model.py, against the road the
project had before (reads filtered by the caller, the whole region piled up, off-target columns masked through
lfq_pileup_skip_snv_columns), against tests/oracle_chain.py::call_targets and against the lines the reference's 2.1.4 binary wrote
(tests/golden/bed_binary.json).  None of the tests reads the reference or its binary.  The caller is shared by the whole suite:
every test takes the targets off the context again."""
import ctypes as C

import numpy as np
import pytest

import bed_edges as be
import bed_model as bm
import golden_util as gu
import maxdepth_model as mm
import util
from test_bed_model import FX, READS, ROWS
from test_gpu_maxdepth import _assert_summary_equal, _fetch, _indel_summary, _tracks_host

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

LFQ_ERR_INVALID = -1


class _Targets:
    """the table of `name` in `text` on the caller's context for the duration of a block"""

    def __init__(self, caller, text, name):
        self.caller, self.text, self.name = caller, text, name

    def __enter__(self):
        import lofreq_amd as la
        bed = la.Bed.parse(self.text)
        self.caller.set_bed(bed, self.name)
        bed.close()                                 # the context keeps its own copy
        return self

    def __exit__(self, *exc):
        self.caller.set_bed(None)


def _query_reads(queries):
    """flat read arrays: read i = [beg, end) of query i as one M operation (a contig of 64 bases: the keep mask reads none)"""
    n = len(queries)
    span = np.array([e - b for b, e in queries], np.int64)
    nb = int(span.sum())
    return {"n": n, "pos": np.array([b for b, _ in queries], np.int32), "cig_off": np.arange(n + 1, dtype=np.int64),
            "cig": (span.astype(np.uint32) << 4), "seq_off": np.concatenate([[0], np.cumsum(span)]).astype(np.int64),
            "seq": np.zeros(nb, np.uint8), "qual": np.full(nb, 30, np.uint8), "mapq": np.full(n, 60, np.uint8),
            "rev": np.zeros(n, np.uint8), "ref": b"A" * 64}


@pytest.mark.parametrize("row", be.ROWS, ids=lambda r: r.name)
def test_kept_reads_equal_the_model(caller, row):
    """every row of tests/bed_edges.py with its queries as reads: as they stand (not sorted) and sorted; sorted, under caps 0, 1, 3"""
    import lofreq_amd as la
    iv = bm.parse(row.text).get(row.contig, [])
    with _Targets(caller, row.text, row.contig):
        for queries in (list(row.queries), sorted(row.queries)):
            pos, ends = [b for b, _ in queries], [e for _, e in queries]
            rs = la.ReadSet.from_arrays(caller, _query_reads(queries))
            try:
                keep, n_kept = rs.kept_reads(None)
                want = bm.keep_reads(iv, pos, ends)
                assert np.array_equal(keep, want), row.name
                assert n_kept == int(want.sum())
                if queries == sorted(row.queries):
                    for d in (0, 1, 3):
                        keep, n_kept = rs.kept_reads(d)
                        want = bm.bed_then_cap(iv, pos, ends, d)
                        assert np.array_equal(keep, want) and n_kept == int(want.sum()), (row.name, d)
            finally:
                rs.close()


def test_unsorted_reads_are_fine_with_a_bed_alone(caller):
    import lofreq_amd as la
    rng = np.random.default_rng(3)
    queries = [(int(p), int(p) + 50) for p in rng.integers(0, 3000, 400)]
    assert queries != sorted(queries)
    R = _query_reads(queries)
    R["ref"] = b"ACGT" * 800
    R["seq"] = rng.integers(0, 4, len(R["seq"])).astype(np.uint8)
    text = "c1\t100\t400\nc1\t1000\t1010\nc1\t2500\t2600\n"
    iv = bm.parse(text)["c1"]
    keep = bm.keep_reads(iv, R["pos"], R["pos"] + 50)
    L = la._lib.load()
    caller.set_pileup_unsorted(True)
    caller.set_pileup_nt_packed(False)
    try:
        with _Targets(caller, text, "c1"):
            rs = la.ReadSet.from_arrays(caller, R)
        got = _tracks_host(caller, rs.pileup_snv(0, 3200))
        cols, col_pos = rs.pileup_indels(0, 3200)
        assert np.array_equal(np.asarray(col_pos), got["col_pos"])
        order = np.argsort(R["pos"], kind="stable")
        sub = la.ReadSet.from_arrays(caller, mm.subset_flat(_reorder(R, order), keep[order]))
        want = _tracks_host(caller, sub.pileup_snv(0, 3200))
        sub.close()
        on = bm.keep_columns(iv, want["col_pos"])
        assert got["col_pos"].tolist() == want["col_pos"][on].tolist() and len(got["col_pos"]) == 300 + 10 + 100
        assert np.array_equal(got["cov"], want["cov"][on]) and np.array_equal(got["nb"], want["nb"][on])
        for c, cw in enumerate(np.nonzero(on)[0]):          # (the read-major kernels hand a column out in no fixed order)
            a, b = int(got["col_off"][c]), int(got["col_off"][c + 1])
            aw, bw = int(want["col_off"][cw]), int(want["col_off"][cw + 1])
            assert sorted(got["nt"][a:b].tolist()) == sorted(want["nt"][aw:bw].tolist())
        # ... and a cap on top is refused, as without targets
        assert L.lfq_set_max_depth(caller.h, 5) == 0
        n = C.c_int64(0)
        assert L.lfq_readset_kept_reads(caller.h, rs.h, None, C.byref(n)) == LFQ_ERR_INVALID
        rs.close()
    finally:
        L.lfq_set_max_depth(caller.h, -1)
        caller.set_pileup_unsorted(False)
        caller.set_pileup_nt_packed(True)
        caller.set_bed(None)


def _reorder(R, order):
    """flat read arrays with the reads in another order"""
    parts = [mm.subset_flat(R, np.arange(R["n"]) == i) for i in order]
    out = dict(R)
    out["pos"] = np.concatenate([p["pos"] for p in parts])
    out["cig"] = np.concatenate([p["cig"] for p in parts])
    out["cig_off"] = np.concatenate([[0], np.cumsum([len(p["cig"]) for p in parts])]).astype(np.int64)
    out["seq_off"] = np.concatenate([[0], np.cumsum([len(p["seq"]) for p in parts])]).astype(np.int64)
    for k in ("seq", "qual"):
        out[k] = np.concatenate([p[k] for p in parts])
    for k in ("mapq", "rev"):
        out[k] = np.concatenate([p[k] for p in parts])
    return out


# ---- equivalence with the road the caller's own BED took ------------------------------------------------------------------------

RB = 200            # region_begin: the region lies inside the contig, so that targets can straddle both of its ends


def _region_reads(width, seed):
    """at most 2 000 reads of 50 bases over a contig of width + 400, planted SNVs and indels; a hole around RB + 1500 with ONE read
    whose deletion alone covers [RB + 1540, RB + 1600)"""
    glen = width + 400
    R = util.make_region_reads(seed, glen, 12 if width < 5000 else 11, rl=50, snv_every=45, indel_every=260, err=0.001)
    assert R["n"] <= 2000
    ends = R["pos"].astype(np.int64) + 55
    hole = (ends > RB + 1500) & (R["pos"] < RB + 1640)
    R = mm.subset_flat(R, ~hole)
    at = int(np.searchsorted(R["pos"], RB + 1520))
    so, co = R["seq_off"], R["cig_off"]
    ins = lambda a, i, v: np.concatenate([a[:i], np.asarray(v, a.dtype), a[i:]])
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    ref = np.frombuffer(R["ref"], np.uint8)
    seq = [code[int(x)] for x in np.concatenate([ref[RB + 1520:RB + 1540], ref[RB + 1600:RB + 1620]])]
    R["pos"] = ins(R["pos"], at, [RB + 1520])
    R["cig"] = ins(R["cig"], int(co[at]), [(20 << 4), (60 << 4) | 2, (20 << 4)])
    R["cig_off"] = np.concatenate([co[:at + 1], co[at:] + 3]).astype(np.int64)
    for k, v in (("seq", seq), ("qual", [38] * 40), ("bi", [70] * 40), ("bd", [70] * 40)):
        R[k] = ins(R[k], int(so[at]), v)
    R["seq_off"] = np.concatenate([so[:at + 1], so[at:] + 40]).astype(np.int64)
    for k, v in (("mapq", 60), ("rev", 0), ("flags", 3)):
        R[k] = ins(R[k], at, [v])
    R["n"] += 1
    return R


def _targets(width):
    re_ = RB + width
    t = [(RB - 30, RB + 40), (RB, RB + 10), (RB + 100, RB + 160), (RB + 64 * 5 - 10, RB + 64 * 5 + 10), (RB + 700, RB + 700),
         (RB + 900, RB + 1300), (RB + 1000, RB + 1100), (RB + 1550, RB + 1560), (RB + 2000, RB + 2001), (RB + 3000, RB + 3900),
         (re_ - 40, re_), (re_ - 5, re_ + 50)]
    if width > 4096:
        t.append((RB + 4096 - 8, RB + 4096 + 8))            # the edge of a compaction tile
        t.append((RB + 5000, RB + 7000))
    return t


def _flat_ends(R):
    co = R["cig_off"]
    return np.array([bm.endpos(int(R["pos"][i]), [("MIDNSHP=X"[int(w) & 15], int(w) >> 4) for w in R["cig"][co[i]:co[i + 1]]])
                     for i in range(R["n"])], np.int64)


def _snv_chain(la, caller, rs, begin, end, conf, cons_of=None, skip=None):
    """pileup_snv + the calls of one region -> (tracks as host arrays, records); cons_of(col_pos) -> the columns whose consensus
    is an indel; skip(col_pos) -> further columns to take out of the SNV pass"""
    dt = rs.pileup_snv(begin, end)
    h = _tracks_host(caller, dt)
    mask = np.zeros(dt.ncols, np.uint8)
    if cons_of is not None:
        mask |= cons_of(dt.col_pos)
    if skip is not None:
        mask |= skip(dt.col_pos)
    if dt.ncols:
        la.skip_snv_columns(caller, mask)
    recs, _, _ = caller.call_snvs(dt, conf)
    return h, recs


def _indel_chain(la, caller, rs, begin, end, conf):
    cols, col_pos = rs.pileup_indels(begin, end)
    recs, _ = la.call_indels(caller, cols, conf)
    items = [(int(col_pos[int(r["col"])]), r, la.format_indel_record("chr1", int(col_pos[int(r["col"])]), cols, r, "PASS").rstrip("\n"))
             for r in recs]
    cons = dict(zip(np.asarray(col_pos).tolist(), np.asarray(cols.cons_indel).tolist()))
    return _indel_summary(cols, col_pos), items, cons


def _lines(la, snv, indel, conf):
    """main_call's epilogue over the records of a run: [(pos0, line)] in position order, indels first within a column"""
    from test_gpu_configs import _snv_lines
    out = []
    for recs, col_pos in snv:
        out += _snv_lines(la, recs, col_pos, conf)
    thr_i = la.snvqual_thresh(conf.sig, conf.bonf_indel)
    out += [(p, 0, line) for p, r, line in indel if int(r["qual"]) >= thr_i]
    return [(t[0], t[2]) for t in sorted(out, key=lambda t: (t[0], t[1]))]


@pytest.mark.parametrize("call_indels", [False, True], ids=["snv", "indels"])
@pytest.mark.parametrize("width", [4095, 4096, 4097, 8193])
def test_bed_on_the_context_equals_the_callers_own_bed(caller, width, call_indels):
    """(a) the targets on the context; (b) none: the reads the model keeps, the whole region piled up, the model's off-target
    columns (and the consensus-indel ones) through lfq_pileup_skip_snv_columns.  lfq_pileup_skip_snv_columns has no twin for the
    indel tests, so with call_indels (b) runs those over each stretch of target positions, one conf carried along."""
    import lofreq_amd as la
    R = _region_reads(width, 700 + width)
    begin, end = RB, RB + width
    targets = _targets(width)
    text = "".join("chr1\t%d\t%d\n" % t for t in targets)
    iv = bm.parse(text)["chr1"]
    keep = bm.keep_reads(iv, R["pos"], _flat_ends(R))
    assert 0 < keep.sum() < R["n"]
    flag = la.LFQ_USE_BAQ | la.LFQ_USE_MQ | (la.LFQ_USE_IDAQ if call_indels else 0)
    caller.set_pileup_nt_packed(False)
    try:
        # ---- (a)
        conf_a = la.VarcallConf(flag=flag)
        with _Targets(caller, text, "chr1"):
            rs = la.ReadSet.from_arrays(caller, R)
        rs.baq(extended=True, idaq=call_indels)
        assert caller.baq_times()["n_reads"] == int(keep.sum())
        got_keep, n_kept = rs.kept_reads(None)
        assert np.array_equal(got_keep, keep) and n_kept == int(keep.sum())
        ind_a, items_a, cons_a = _indel_chain(la, caller, rs, begin, end, conf_a) if call_indels else (None, [], {})
        h_a, recs_a = _snv_chain(la, caller, rs, begin, end, conf_a,
                                 cons_of=lambda cp: np.array([cons_a.get(int(p), 0) for p in cp], np.uint8))
        summ = rs.plp_summary(begin, end)
        assert np.asarray(summ.col_pos).tolist() == h_a["col_pos"].tolist()
        rs.close()
        lines_a = _lines(la, [(recs_a, h_a["col_pos"])], items_a, conf_a)
        # ---- (b)
        conf_b = la.VarcallConf(flag=flag)
        sub = la.ReadSet.from_arrays(caller, mm.subset_flat(R, keep))
        sub.baq(extended=True, idaq=call_indels)
        items_b, cons_b, ind_cols = [], {}, []
        on_pos = [p for p in range(begin, end) if bm.overlap(iv, p, p + 1)]
        runs, start = [], None
        for p in on_pos + [None]:
            if start is None:
                start = prev = p
            elif p is None or p != prev + 1:
                runs.append((start, prev + 1))
                start = prev = p
            else:
                prev = p
        if call_indels:
            for lo, hi in runs:
                summ_b, it, cons = _indel_chain(la, caller, sub, lo, hi, conf_b)
                items_b += it
                cons_b.update(cons)
                ind_cols += summ_b["col_pos"].tolist()
        h_b, recs_b = _snv_chain(la, caller, sub, begin, end, conf_b,
                                 cons_of=lambda cp: np.array([cons_b.get(int(p), 0) for p in cp], np.uint8),
                                 skip=lambda cp: (~bm.keep_columns(iv, cp)).astype(np.uint8))
        sub.close()
        on = bm.keep_columns(iv, h_b["col_pos"])
        # the same columns, the same tracks per column
        assert h_a["col_pos"].tolist() == h_b["col_pos"][on].tolist() and 0 < on.sum() < len(on)
        assert RB + 1555 in h_a["col_pos"].tolist() and RB + 1545 not in h_a["col_pos"].tolist()    # covered by the deletion only
        assert RB + 700 not in h_a["col_pos"].tolist()
        for k in ("ref_base", "cov"):
            assert np.array_equal(h_a[k], h_b[k][on]), k
        cols_b = np.nonzero(on)[0]
        for c, cb in enumerate(cols_b):
            a, b = int(h_a["col_off"][c]), int(h_a["col_off"][c + 1])
            a2, b2 = int(h_b["col_off"][cb]), int(h_b["col_off"][cb + 1])
            assert b - a == b2 - a2
            for k in ("nt", "bq", "baq", "mq"):
                assert np.array_equal(h_a[k][a:b], h_b[k][a2:b2]), (k, c)
        if call_indels:
            assert ind_a["col_pos"].tolist() == h_a["col_pos"].tolist() == ind_cols
        # the same records, lines and test counts
        lines_b = _lines(la, [(recs_b, h_b["col_pos"])], items_b, conf_b)
        assert lines_a == lines_b and len(lines_a) >= 5
        assert conf_a.num_snv_tests == conf_b.num_snv_tests and conf_a.num_indel_tests == conf_b.num_indel_tests
        assert conf_a.bonf_subst == conf_b.bonf_subst and conf_a.bonf_indel == conf_b.bonf_indel
        assert len(recs_a) == len(recs_b)
        for ra, rb in zip(recs_a, recs_b):
            assert int(h_a["col_pos"][int(ra["col"])]) == int(h_b["col_pos"][int(rb["col"])]) and int(ra["qual"]) == int(rb["qual"])
            util.assert_pvalue_close(ra["pvalue"], rb["pvalue"], ctx="col %d" % int(ra["col"]))
        assert [(p, int(r["qual"]), int(r["count"])) for p, r, _ in items_a] == [(p, int(r["qual"]), int(r["count"])) for p, r, _ in items_b]
        for (_, ra, _), (_, rb, _) in zip(items_a, items_b):
            util.assert_pvalue_close(ra["pvalue"], rb["pvalue"], ctx="indel")
    finally:
        caller.set_pileup_nt_packed(True)
        caller.set_bed(None)


# ---- the oracle and the binary -------------------------------------------------------------------------------------------------

def test_lines_equal_the_oracles_call_targets(caller, oracle):
    import lofreq_amd as la
    import oracle_chain as oc
    from test_gpu_configs import _snv_lines
    glen = 5000
    R = util.make_region_reads(77, glen, 12, rl=50, snv_every=45, indel_every=9000, err=0.001)     # (one indel site, at 3000: in no target)
    targets = [("chr1", 0, 120), ("chr1", 300, 301), ("chr1", 640, 1500), ("chr1", 2000, 2064), ("chr1", 4090, 4100), ("chr1", 4900, glen)]
    text = "".join("%s\t%d\t%d\n" % t for t in targets)
    conf = la.VarcallConf()
    with _Targets(caller, text, "chr1"):
        rs = la.ReadSet.from_arrays(caller, R)
    rs.baq(extended=True, idaq=False)
    dt = rs.pileup_snv(0, glen)
    recs, _, _ = caller.call_snvs(dt, conf)
    rs.close()
    P = dict(R)
    oracle.baq_idaq_reads(P, extended=True, idaq=False, procs=1)
    ref = oc.call_targets(oracle, P, R["ref"], targets, dict(flag=la.LFQ_USE_BAQ | la.LFQ_USE_MQ))
    assert dt.ncols == ref["n_columns"] and conf.num_snv_tests == ref["n_snv_tests"] and conf.bonf_subst == ref["conf"].bonf_subst
    assert [l[2] for l in _snv_lines(la, recs, dt.col_pos, conf)] == ref["lines"] and len(ref["lines"]) >= 5
    assert len(recs) == len(ref["emitted"])
    for r, (p0, pv) in zip(recs, ref["emitted"]):
        assert int(dt.col_pos[int(r["col"])]) == p0
        util.assert_pvalue_close(r["pvalue"], pv, ctx="pos %d" % p0)


def _fixture_run(la, caller, text, max_depth):
    """both contigs of the fixture under the targets of `text`, one conf carried from contig to contig -> (lines, columns, conf)"""
    from test_gpu_configs import _snv_lines
    conf = la.VarcallConf()
    per, cols = [], {}
    for name, _ in FX["contigs"]:
        ref = FX["genome"][name].encode()
        with _Targets(caller, text, name):
            rs = la.ReadSet(caller, READS[name], ref)
        rs.baq(extended=True, idaq=False)
        dt = rs.pileup_snv(0, len(ref), max_depth=max_depth)
        recs, _, _ = caller.call_snvs(dt, conf)
        rs.close()
        per.append((name, recs, dt.col_pos))
        cols[name] = np.asarray(dt.col_pos).tolist()
    lines = []
    for name, recs, col_pos in per:
        lines += [l[2] for l in _snv_lines(la, recs, col_pos, conf, chrom=name)]
    return lines, cols, conf


@pytest.mark.parametrize("name", [b["name"] for b in FX["beds"] if b["status"] == 0])
def test_fixture_columns_and_lines_are_the_binarys(caller, name):
    import lofreq_amd as la
    from test_bed_model import unpack
    row = ROWS[name]
    runs = row.get("calls") or [{"max_depth": None, "columns": row["columns"]}]
    for run in runs:
        lines, cols, conf = _fixture_run(la, caller, row["text"], run["max_depth"])
        want, _ = unpack(run["columns"])
        assert {k: v for k, v in cols.items() if v} == want, (name, run["max_depth"])
        if "vcf" in run:
            assert lines == [gu.strip_hqa(l) for l in run["vcf"]] and conf.num_snv_tests == run["num_snv_tests"], (name, run["max_depth"])


# ---- empty cases, BAQ, binding at creation --------------------------------------------------------------------------------------

def test_empty_tables_return_no_columns_and_launch_nothing(caller):
    import lofreq_amd as la
    ref = FX["genome"]["c1"].encode()
    for text, name in (("# no line at all\n", "c1"), ("c2\t0\t400\n", "c1"), ("c1\t590\t600\n", "c1")):
        with _Targets(caller, text, name):
            rs = la.ReadSet(caller, READS["c1"], ref)
        keep, n_kept = rs.kept_reads(None)
        assert n_kept == 0 and not keep.any()
        rs.baq(extended=True, idaq=True)
        assert caller.baq_times()["n_reads"] == 0 and caller.baq_times()["n_launches"] == 0
        lb, ai, ad, fl = rs.fetch_tags(idaq=True)
        assert not lb.any() and not fl.any()
        assert rs.pileup_snv(0, len(ref)).ncols == 0
        cols, col_pos = rs.pileup_indels(0, len(ref))
        assert cols.ncols == 0 and len(col_pos) == 0
        assert rs.plp_summary(0, len(ref)).ncols == 0
        rs.close()


def test_baq_runs_for_the_kept_reads_and_a_read_set_keeps_the_bed_it_was_created_under(caller):
    import lofreq_amd as la
    ref = FX["genome"]["c1"].encode()
    reads = READS["c1"]
    text = ROWS["plain"]["text"]
    iv = bm.parse(text)["c1"]
    keep = bm.keep_reads(iv, [r["pos0"] for r in reads], [bm.endpos(r["pos0"], r["cigar"]) for r in reads])
    before = la.ReadSet(caller, reads, ref)                     # created before lfq_set_bed: takes every read, whatever follows
    with _Targets(caller, text, "c1"):
        rs = la.ReadSet(caller, reads, ref)
        before.baq(extended=True, idaq=True)
        assert caller.baq_times()["n_reads"] == len(reads)
        assert before.kept_reads(None)[1] == len(reads)
        full = before.pileup_snv(0, len(ref))
        assert full.ncols > sum(e - b for b, e in iv)
    # ... and the other way round: the targets are off the context, the read set created under them still has them
    rs.baq(extended=True, idaq=True)
    assert caller.baq_times()["n_reads"] == int(keep.sum()) and 0 < keep.sum() < len(reads)
    lb, ai, ad, fl = rs.fetch_tags(idaq=True)
    lb0, ai0, ad0, fl0 = before.fetch_tags(idaq=True)
    so = np.concatenate([[0], np.cumsum([len(r["seq"]) for r in reads])])
    for i, k in enumerate(keep):
        a, b = int(so[i]), int(so[i + 1])
        if k:
            assert np.array_equal(lb[a:b], lb0[a:b]) and np.array_equal(ai[a:b], ai0[a:b]) and np.array_equal(ad[a:b], ad0[a:b])
            assert fl[i] == fl0[i]
        else:
            assert not lb[a:b].any() and (ai[a:b] == ord("~")).all() and (ad[a:b] == ord("~")).all() and fl[i] == 0
    assert fl0.any()
    got = rs.pileup_snv(0, len(ref))
    assert got.col_pos.tolist() == [p for p in full.col_pos.tolist() if bm.overlap(iv, p, p + 1)]
    # lofreq uniq has no -l: the sites pileup takes every read
    t, cov, _ = rs.pileup_sites([10, 130, 400])
    t0, cov0, _ = before.pileup_sites([10, 130, 400])
    assert cov.tolist() == cov0.tolist() and cov[0] > 0
    rs.close()
    before.close()


def test_without_a_bed_the_pileups_are_byte_equal_to_before_the_first_set_bed(tmp_path):
    """a context of its own: the three pileups before lfq_set_bed was ever called on it, and after targets were set and taken off"""
    import lofreq_amd as la
    c = la.SnvCaller(0)
    c.set_pileup_nt_packed(False)
    try:
        ref = FX["genome"]["c1"].encode()

        def run():
            rs = la.ReadSet(c, READS["c1"], ref)
            rs.baq(extended=True, idaq=True)
            h = _tracks_host(c, rs.pileup_snv(0, len(ref)))
            ind = _indel_summary(*rs.pileup_indels(0, len(ref)))
            s = rs.plp_summary(0, len(ref))
            summ = {k: np.asarray(getattr(s, k)).copy() for k in ("col_pos", "fw", "rv", "num_heads", "num_tails", "coverage_plp")}
            rs.close()
            return h, ind, summ

        h0, i0, s0 = run()
        with _Targets(c, ROWS["plain"]["text"], "c1"):
            h1, _, _ = run()
        assert len(h1["col_pos"]) < len(h0["col_pos"])
        h2, i2, s2 = run()
        for k in h0:
            assert np.array_equal(np.asarray(h0[k]), np.asarray(h2[k])), k
        _assert_summary_equal(i0, i2)
        for k in s0:
            assert np.array_equal(s0[k], s2[k]), k
    finally:
        c.close()


# ---- the region binding ---------------------------------------------------------------------------------------------------------

def _region_run(caller, lib, text, road, conf):
    """both contigs of the fixture, a region each, every read of the contig fed (the caller filters nothing), lfq_region_set_bed"""
    import bam_records as br
    import bgzf_edges as bz
    import lofreq_amd as la
    import test_gpu_chain as tc
    P = C.CDLL(lib)
    lines = []
    EMIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)
    cb = EMIT(lambda user, s: lines.append(s.decode().rstrip("\n")))
    o = tc._RegionOpts()
    P.lfq_region_opts_init(C.byref(o))
    h = C.c_void_p()
    P.lfq_region_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, EMIT, C.c_void_p]
    assert P.lfq_region_open(C.byref(h), caller.h, C.byref(conf.c), C.byref(o), cb, None) == 0
    P.lfq_region_set_bed.argtypes = [C.c_void_p, C.c_void_p]
    bed = la.Bed.parse(text)
    assert P.lfq_region_set_bed(h, bed.h) == 0
    P.lfq_region_begin.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int64]
    P.lfq_region_add_read.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_char_p, C.c_char_p]
    P.lfq_region_add_record.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
    P.lfq_region_add_bgzf.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_int64, C.c_int64, C.c_int64]
    P.lfq_region_end.argtypes = [C.c_void_p]
    P.lfq_region_close.argtypes = [C.c_void_p, C.c_void_p]
    keep_alive = []
    for tid, (name, n) in enumerate(FX["contigs"]):
        ref = FX["genome"][name].encode()
        keep_alive.append(ref)
        assert P.lfq_region_begin(h, name.encode(), ref, len(ref), 0, n) == 0
        assert P.lfq_region_set_bed(h, bed.h) == LFQ_ERR_INVALID        # a region is open
        reads = READS[name]
        if road == "bgzf":
            header = b"BAM\1" + b"t" * 41
            payload = header + b"".join(bz.bam_record(dict(r, name="read%d" % i), tid) for i, r in enumerate(reads))
            comp = bz.bgzf_blocks(payload, range(1501, len(payload), 1501)) + bz.EOF_BLOCK
            assert P.lfq_region_add_bgzf(h, tid, comp, len(comp), len(header), -1) == 0
        for i, r in enumerate(reads if road != "bgzf" else []):
            flag = 16 if r["reverse"] else 0
            if road == "record":
                lq, nc, ls, data = br.record_fields(dict(r, name="read%d" % i))
                rc = P.lfq_region_add_record(h, r["pos0"], flag, r["mapq"], lq, nc, ls, data, len(data))
            else:
                seq4, cig, bi, bd = tc._bam_fields(r)
                q = np.asarray(r["qual"], np.uint8)
                rc = P.lfq_region_add_read(h, r["pos0"], flag, r["mapq"], len(cig), cig.ctypes.data, len(q), seq4.ctypes.data,
                                           q.ctypes.data, bi, bd)
            assert rc in (0, 1)
        assert P.lfq_region_end(h) == 0
    assert P.lfq_region_close(h, None) == 0
    bed.close()
    return lines


@pytest.mark.parametrize("road", ["read", "record", "bgzf"])
def test_region_binding_takes_the_bed(caller, tmp_path, road):
    import lofreq_amd as la
    import test_gpu_chain as tc
    lib = tc._build_region_lib(tmp_path)
    for name in ("plain", "both_formats", "contig_without_line"):
        row = ROWS[name]
        run = [r for r in row["calls"] if r["max_depth"] is None][0]
        conf = la.VarcallConf()
        lines = _region_run(caller, lib, row["text"], road, conf)
        assert conf.num_snv_tests == run["num_snv_tests"], (name, road)
        assert tc._epilogue(la, lines, conf) == [gu.strip_hqa(l) for l in run["vcf"]], (name, road)
        want, _, conf_a = _fixture_run(la, caller, row["text"], None)
        assert tc._epilogue(la, lines, conf) == want and conf.bonf_subst == conf_a.bonf_subst
    # close took the targets off the context: a read set created now takes every read
    rs = la.ReadSet(caller, READS["c1"], FX["genome"]["c1"].encode())
    assert rs.kept_reads(None)[1] == len(READS["c1"])
    rs.close()
