"""-m gpu: plp_summary's header line on the device (lfq_readset_plp_summary + lfq_format_plp_summary) -- byte for byte against the
lines the reference's 2.1.4 binary printed (tests/golden/plpsummary_*.json) and against every row of the edge table
(tests/plpsummary_edges.py, held to the restatement and through it to the binary by the CPU tests); the consensus flag, the
counts shared with the indel pileup, the path the kernel took on the tie rows, and the SNV tracks left alone."""
import ctypes as C

import numpy as np
import pytest

import plpsummary_edges as E
import plpsummary_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROWS = E.table()


def _fetch(ptr, nbytes):
    """device memory at a raw pointer -> numpy"""
    hip = C.CDLL("libamdhip64.so")
    out = np.zeros(max(nbytes, 1), np.uint8)
    if nbytes:
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0   # DeviceToHost
    return out[:nbytes]


def _agrees_with_the_indel_pileup(rs, s, begin, end, min_plp_idq=0, max_depth=None):
    cols, col_pos = rs.pileup_indels(begin, end, min_plp_idq=min_plp_idq, max_depth=max_depth)
    assert s.ncols == cols.ncols and s.col_pos.tolist() == col_pos.tolist()
    assert ((s.cons_kind != 0) == (cols.cons_indel != 0)).all()
    for a, b in (("num_tails", "num_tails"), ("num_ins", "num_ins"), ("num_dels", "num_dels"), ("hrun", "hrun"),
                 ("coverage_plp", "coverage_plp")):
        assert np.array_equal(getattr(s, a), getattr(cols, b)), a
    assert np.array_equal(s.ref_base, cols.ref_base)


@pytest.mark.parametrize("name", ("plpsummary_snv", "plpsummary_indel"))
def test_goldens_give_the_lines_of_the_binary(caller, name):
    import lofreq_amd as la
    fx, reads = ref.load_golden(name)
    genome = fx["genome"].encode()
    rs = la.ReadSet(caller, reads, genome)
    try:
        s = rs.plp_summary(0, len(genome))
        got = la.format_plp_summary(fx["chrom"], s)
        assert len(got) == len(fx["lines"])
        for g, w in zip(got, fx["lines"]):
            assert g == w
        ts = rs.last_summary_times()
        assert ts.n_launches == 1 and ts.n_cols == s.ncols == len(got) and ts.kernel_ms > 0 and 0 <= ts.n_ordered <= ts.n_cols
        assert [c[0] for c in s.cons] == [l.split("\t")[3][0] for l in fx["lines"]]
        _agrees_with_the_indel_pileup(rs, s, 0, len(genome))
    finally:
        rs.close()


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_edge_rows(caller, row):
    import lofreq_amd as la
    rs = la.ReadSet(caller, row.reads, row.ref.encode())
    try:
        s = rs.plp_summary(row.begin, row.end, min_plp_bq=row.min_plp_bq, min_plp_idq=row.min_plp_idq, max_depth=row.max_depth)
        got = la.format_plp_summary(E.CHROM, s)
        assert s.col_pos.tolist() == sorted(row.expect)
        assert dict(zip(s.col_pos.tolist(), got)) == row.expect
        ts = rs.last_summary_times()
        assert ts.n_cols == s.ncols and ts.n_launches == (1 if s.ncols else 0)
        if row.ordered == "some":
            assert ts.n_ordered >= 1
        elif row.ordered == "none":
            assert ts.n_ordered == 0
        _agrees_with_the_indel_pileup(rs, s, row.begin, row.end, row.min_plp_idq, row.max_depth)
    finally:
        rs.close()


def test_snv_tracks_are_untouched_by_the_summary_call(caller):
    import lofreq_amd as la
    fx, reads = ref.load_golden("plpsummary_indel")
    genome = fx["genome"].encode()
    rs = la.ReadSet(caller, reads, genome)
    try:
        dt = rs.pileup_snv(0, len(genome), sync=True)
        t = dt._tracks()
        n = int(t.ncols)

        def snapshot():
            off = _fetch(t.col_off, (n + 1) * 8).view(np.uint64)
            n_obs = int(off[-1])
            nt_bytes = (n_obs + 7) // 8 * 4 if t.flags & 1 else n_obs        # LFQ_TRACKS_NT_PACKED
            return [off.copy(), _fetch(t.nt, nt_bytes), _fetch(t.bq, n_obs), _fetch(t.baq, n_obs), _fetch(t.mq, n_obs),
                    _fetch(t.ref_base, n), _fetch(t.coverage_plp, n * 4), _fetch(t.num_bases, n * 4)]

        before = snapshot()
        assert n > 300 and int(before[0][-1]) > 10000
        s = rs.plp_summary(0, len(genome))
        assert s.ncols == n and s.col_pos.tolist() == dt.col_pos.tolist()
        after = snapshot()
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        # the kept bases of the tracks are the bases the summary counted
        nb = after[7].view(np.int32)
        assert np.array_equal(nb, s.fw.sum(axis=1) + s.rv.sum(axis=1))
    finally:
        rs.close()


def test_refusals_and_empty_cases(caller):
    import lofreq_amd as la
    from lofreq_amd import _lib
    fx, reads = ref.load_golden("plpsummary_snv")
    genome = fx["genome"].encode()
    L = _lib.load()
    out = C.POINTER(_lib.PlpSummaryC)()
    rs = la.ReadSet(caller, reads, genome)
    try:
        call = lambda b, e, bq=3: L.lfq_readset_plp_summary(caller.h, rs.h, b, e, bq, 0, C.byref(out))
        assert call(10, 9) == -1 and call(-1, 10) == -1 and call(0, len(genome) + 1) == -1 and call(0, 10, -1) == -1
        assert L.lfq_readset_plp_summary(caller.h, rs.h, 0, 10, 3, 0, None) == -1
        assert call(5, 5) == 0 and out.contents.ncols == 0
        assert rs.last_summary_times().n_launches == 0
        assert call(0, len(genome)) == 0 and out.contents.ncols == len(fx["lines"])
    finally:
        rs.close()
    # reads that are not position-sorted: refused, whatever lfq_set_pileup_unsorted says
    swapped = [reads[50], reads[0]] + reads[51:60]
    assert swapped[0]["pos0"] > swapped[1]["pos0"]
    rs = la.ReadSet(caller, swapped, genome)
    try:
        assert L.lfq_set_pileup_unsorted(caller.h, 1) == 0
        assert L.lfq_readset_plp_summary(caller.h, rs.h, 0, len(genome), 3, 0, C.byref(out)) == -1
    finally:
        L.lfq_set_pileup_unsorted(caller.h, 0)
        rs.close()
    # no read covers the region
    rs = la.ReadSet(caller, [E.rd(10, "4M", "GCTT", 30)], E.REF.encode())
    try:
        s = rs.plp_summary(30, 40)
        assert s.ncols == 0 and la.format_plp_summary("x", s) == [] and rs.last_summary_times().n_launches == 0
    finally:
        rs.close()
