"""-m gpu: the quality lines of plp_summary on the device (lfq_plp_quals_from_tracks, lfq_plp_group_kernel, the all-columns
switch of the indel pileup, the two formatters, ReadSet.plpsummary_text) -- byte for byte against the complete text the
reference's 2.1.4 binary printed (tests/golden/plpquals_*.json) and against every row of the edge table (tests/plpquals_edges.py,
held to the restatement and through it to the binary by the CPU tests)."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
import plpquals_edges as E
import plpquals_ref as Q

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROWS = E.table()
TRACK_ROWS = [r for r in ROWS if isinstance(r, E.TrackRow)]
READ_ROWS = [r for r in ROWS if isinstance(r, E.ReadRow)]


def _fetch(ptr, nbytes):
    """device memory at a raw pointer -> numpy"""
    hip = C.CDLL("libamdhip64.so")
    out = np.zeros(max(nbytes, 1), np.uint8)
    if nbytes:
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0   # DeviceToHost
    return out[:nbytes]


def _untagged(reads):
    """the reads without what `lofreq alnqual` added: the read set computes lb / ai / ad itself"""
    return [{k: v for k, v in r.items() if k not in ("lb", "ai", "ad")} for r in reads]


def _same(a, b):
    assert a.ncols == b.ncols and a.col_begin == b.col_begin and a.nt_off.tolist() == b.nt_off.tolist()
    for n in ("bq", "baq", "mq", "sq"):
        x, y = getattr(a, n), getattr(b, n)
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), n


@pytest.fixture(scope="module")
def indel_set(caller):
    """plpquals_indel as a resident read set with BAQ / IDAQ, its byte-nt SNV tracks and the grouped qualities of all columns"""
    import lofreq_amd as la
    fx, reads, blocks = Q.load_golden("plpquals_indel")
    genome = fx["genome"].encode()
    rs = la.ReadSet(caller, _untagged(reads), genome)
    rs.baq(idaq=True)
    caller.set_pileup_nt_packed(False)
    try:
        dt = rs.pileup_snv(0, len(genome), sync=True)
    finally:
        caller.set_pileup_nt_packed(True)
    yield fx, rs, dt, la.plp_quals(caller, dt)
    rs.close()


@pytest.mark.parametrize("name", ("plpquals_indel", "plpquals_srcq", "plpquals_deep"))
def test_goldens_give_the_text_of_the_binary(caller, name):
    import lofreq_amd as la
    fx, reads, blocks = Q.load_golden(name)
    genome = fx["genome"].encode()
    flag = Q.flag_of(fx)
    rs = la.ReadSet(caller, _untagged(reads), genome)
    try:
        rs.baq(idaq=True)
        if flag & Q.LFQ_USE_SQ:
            rs.source_qual()
        got = rs.plpsummary_text(fx["chrom"], 0, len(genome), flag)
        assert len(got) == len(blocks)
        for g, w in zip(got, blocks):
            assert g == w
        assert "".join(got) == fx["text"]
    finally:
        rs.close()


@pytest.mark.parametrize("row", TRACK_ROWS, ids=[r.name for r in TRACK_ROWS])
def test_track_rows(caller, row):
    import lofreq_amd as la
    host = la.PileupBatch(row.nt, row.bq, row.mq, row.col_off, np.full(len(row.col_off) - 1, ord("A"), np.uint8), baq=row.baq,
                          sq=row.sq)
    q = la.plp_quals(caller, host, row.c0, row.c1)
    nt_off, bq, baq, mq, sq = row.expect
    assert q.ncols == row.c1 - row.c0 and q.col_begin == row.c0
    assert q.nt_off.tolist() == nt_off
    assert q.bq.tolist() == bq and q.mq.tolist() == mq
    assert (q.baq is None and baq is None) or q.baq.tolist() == baq
    assert (q.sq is None and sq is None) or q.sq.tolist() == sq
    assert la.format_plp_quals(q, row.flag) == row.text
    ts = la.last_plp_quals_times(caller)
    assert ts.n_cols == q.ncols and ts.n_obs == nt_off[-1] and ts.n_launches == (1 if nt_off[-1] else 0)
    assert (ts.kernel_ms > 0) == (ts.n_launches == 1)


@pytest.mark.parametrize("row", READ_ROWS, ids=[r.name for r in READ_ROWS])
def test_read_rows(caller, row):
    import lofreq_amd as la
    rs = la.ReadSet(caller, row.reads, row.ref.encode())
    try:
        got = rs.plpsummary_text(E.CHROM, row.begin, row.end, row.flag, min_plp_bq=row.min_plp_bq, min_plp_idq=row.min_plp_idq,
                                 max_depth=row.max_depth)
        assert got == row.expect
    finally:
        rs.close()


def test_group_sizes_are_the_counts_of_the_summary(caller, indel_set):
    fx, rs, dt, q = indel_set
    s = rs.plp_summary(0, len(fx["genome"]))
    assert q.ncols == s.ncols == dt.ncols > 100
    assert np.array_equal(np.diff(q.nt_off).reshape(-1, 5), s.fw + s.rv)


def test_host_tracks_give_what_resident_tracks_give(caller, indel_set):
    import lofreq_amd as la
    fx, rs, dt, q = indel_set
    t = dt._tracks()
    n = int(t.ncols)
    off = _fetch(t.col_off, (n + 1) * 8).view(np.uint64).copy()
    n_obs = int(off[-1])
    assert not t.flags & 1 and n_obs > 1000
    host = la.PileupBatch(_fetch(t.nt, n_obs), _fetch(t.bq, n_obs), _fetch(t.mq, n_obs), off, _fetch(t.ref_base, n),
                          baq=_fetch(t.baq, n_obs))
    _same(la.plp_quals(caller, host), q)
    _same(la.plp_quals(caller, host, 7, n - 5), la.plp_quals(caller, dt, 7, n - 5))


def test_two_half_ranges_are_the_whole_range(caller, indel_set):
    import lofreq_amd as la
    fx, rs, dt, q = indel_set
    mid = dt.ncols // 2 + 1
    a, b = la.plp_quals(caller, dt, 0, mid), la.plp_quals(caller, dt, mid, dt.ncols)
    assert a.col_begin == 0 and b.col_begin == mid and a.ncols + b.ncols == q.ncols
    assert a.nt_off.tolist() + (b.nt_off[1:] + a.nt_off[-1]).tolist() == q.nt_off.tolist()
    for n in ("bq", "baq", "mq"):
        assert np.concatenate([getattr(a, n), getattr(b, n)]).tobytes() == getattr(q, n).tobytes()
    flag = Q.LFQ_USE_BAQ
    assert la.format_plp_quals(a, flag) + la.format_plp_quals(b, flag) == la.format_plp_quals(q, flag)


def test_snv_tracks_are_untouched_and_an_empty_range_launches_nothing(caller, indel_set):
    import lofreq_amd as la
    fx, rs, dt, q = indel_set
    t = dt._tracks()
    n = int(t.ncols)

    def snapshot():
        off = _fetch(t.col_off, (n + 1) * 8).view(np.uint64)
        n_obs = int(off[-1])
        return [off.copy(), _fetch(t.nt, n_obs), _fetch(t.bq, n_obs), _fetch(t.baq, n_obs), _fetch(t.mq, n_obs),
                _fetch(t.ref_base, n), _fetch(t.coverage_plp, n * 4), _fetch(t.num_bases, n * 4)]

    before = snapshot()
    _same(la.plp_quals(caller, dt), q)
    assert la.last_plp_quals_times(caller).n_launches == 1
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    e = la.plp_quals(caller, dt, 5, 5)
    ts = la.last_plp_quals_times(caller)
    assert e.ncols == 0 and e.col_begin == 5 and e.nt_off.tolist() == [0] and len(e.bq) == 0
    assert ts.n_launches == 0 and ts.kernel_ms == 0 and ts.n_cols == 0 and ts.n_obs == 0
    assert la.format_plp_quals(e, Q.LFQ_USE_BAQ) == []


def test_refusals(caller, indel_set):
    import lofreq_amd as la
    from lofreq_amd import _lib
    fx, rs, dt, q = indel_set
    L = _lib.load()
    out = C.POINTER(_lib.PlpQualsC)()
    t = dt._tracks()
    call = lambda tr, b, e: L.lfq_plp_quals_from_tracks(caller.h, C.byref(tr), 1, b, e, C.byref(out))
    assert call(t, 3, 2) == -1 and call(t, -1, 2) == -1 and call(t, 0, dt.ncols + 1) == -1
    assert L.lfq_plp_quals_from_tracks(caller.h, C.byref(t), 1, 0, 1, None) == -1
    packed = _lib.Tracks()                                  # the same tracks declared LFQ_TRACKS_NT_PACKED: refused by the flag
    C.memmove(C.byref(packed), C.byref(t), C.sizeof(packed))
    packed.flags = _lib.LFQ_TRACKS_NT_PACKED
    assert call(packed, 0, 1) == -1
    assert call(packed, 0, 0) == -1
    _same(la.plp_quals(caller, dt), q)                      # and the context still answers


def test_all_columns_switch_leaves_the_indel_calls_alone():
    """a context that never saw the switch, then the switch on, then off again: the records of lfq_call_indels_batch are the
    same three times, the ne_off of the off runs are identical, and with it on every column has its arrays"""
    import lofreq_amd as la
    caller = la.SnvCaller(0)
    try:
        fx, reads = gu.load_plpindel(gu.GOLDEN_DIR + "/plpindel_default.json")
        ref = fx["genome"].encode()
        kw, _ = gu.conf_kwargs(fx["call_args"])

        def run():
            cols, col_pos = la.pileup_indel_columns(caller, reads, ref, 0, len(ref))
            recs, nt = la.call_indels(caller, cols, la.VarcallConf(**kw))
            return cols, col_pos, recs, nt

        c0, p0, r0, n0 = run()                               # before the switch was ever touched
        caller.set_indel_arrays_all_columns(True)
        c1, p1, r1, n1 = run()
        caller.set_indel_arrays_all_columns(False)
        c2, p2, r2, n2 = run()
        assert len(r0) > 0 and n0 == n1 == n2 and p0.tolist() == p1.tolist() == p2.tolist()
        assert r0.tobytes() == r1.tobytes() == r2.tobytes()
        for sd in range(2):
            a, b, c = c0.sides[sd], c1.sides[sd], c2.sides[sd]
            for k in a:
                assert a[k].tobytes() == c[k].tobytes(), k
            cnt = a["non_fw"] + a["non_rv"]
            assert np.array_equal(np.diff(b["ne_off"]), cnt) and int(b["ne_off"][-1]) > int(a["ne_off"][-1])
            assert not np.array_equal(np.diff(a["ne_off"]), cnt)              # today: only at columns with an event
            for k in ("non_fw", "non_rv", "ev_off", "key_off", "rd_off", "rd_q", "rd_aq", "rd_mq", "rd_sq"):
                assert a[k].tobytes() == b[k].tobytes(), k
            # where the default run has a column's arrays, the all-columns run has the same values
            for col in np.flatnonzero(np.diff(a["ne_off"]))[:50]:
                for k in ("ne_q", "ne_mq"):
                    assert a[k][a["ne_off"][col]:a["ne_off"][col + 1]].tolist() == b[k][b["ne_off"][col]:b["ne_off"][col + 1]].tolist()
        # the formatter refuses the columns of the off run that lack their arrays, and device-only arrays
        from lofreq_amd import _lib
        L = _lib.load()
        cs = c0.c_struct()
        col = int(np.flatnonzero((np.diff(c0.sides[0]["ne_off"]) == 0) & (c0.sides[0]["non_fw"] + c0.sides[0]["non_rv"] > 0))[0])
        assert L.lfq_format_plp_indel_quals(None, 0, C.byref(cs), col) == -1
        assert len(la.format_plp_indel_quals(c1)) == c1.ncols
    finally:
        caller.close()
