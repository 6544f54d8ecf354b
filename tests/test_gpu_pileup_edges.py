"""-m gpu: the pileup tile kernels at their row, round and tile boundaries (tests/pileup_edges.py).

Every row of the table runs through lfq_pileup_snv_tracks in both nt layouts -- column positions and offsets, coverage_plp,
num_bases, the reference bytes, max_col_obs and the nt / bq / baq / mq tracks in pileup order, byte for byte against the oracle's
column builder -- and through lfq_pileup_indel_columns, every field against golden_util.py_indel_pileup.  Once per group the same
rows go through a resident read set, whose kernel arguments lfq_readset.hip assembles."""
import os

import numpy as np
import pytest

import golden_util as gu
import pileup_edges as pe
from test_gpu_pileup import _fetch, _fetch_nt

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TABLE = pe.boundary_table()
BY_NAME = {r.name: r for r in TABLE}
_INDEL = {}


def _indel_ref(row):
    if row.name not in _INDEL:
        _INDEL[row.name] = gu.py_indel_pileup(row.reads, row.ref, min_plp_idq=row.min_plp_idq)
    return _INDEL[row.name]


def _lb(row):
    return None if row.reads[0]["lb"] is None else [r["lb"] for r in row.reads]


def _check_snv(dt, packed, out, ctx):
    """device tracks against orc_pileup_region's"""
    t = dt._tracks()
    ncols = dt.ncols
    h = out["host"]
    assert bool(t.flags & 1) == packed, ctx
    assert ncols == len(out["col_pos"]) and np.array_equal(np.asarray(dt.col_pos[:ncols]), out["col_pos"]), ctx
    if ncols == 0:
        assert int(t.max_col_obs) == 0, ctx
        return
    off = _fetch(t.col_off, (ncols + 1) * 8).view(np.uint64)
    assert np.array_equal(off, h["col_off"]), ctx
    n_obs = int(off[-1])
    cov = _fetch(t.coverage_plp, max(ncols, 1) * 4).view(np.int32)[:ncols]
    nb = _fetch(t.num_bases, max(ncols, 1) * 4).view(np.int32)[:ncols]
    ref = _fetch(t.ref_base, max(ncols, 1))[:ncols]
    assert np.array_equal(cov, h["coverage_plp"]) and np.array_equal(nb, h["num_bases"]), ctx
    assert np.array_equal(ref, h["ref_base"][:ncols]), ctx
    assert int(t.max_col_obs) == (int(nb.max()) if ncols else 0) == dt.max_col_obs, ctx
    got = {"nt": _fetch_nt(t, n_obs)}
    got.update({k: _fetch(p, max(n_obs, 1))[:n_obs] for k, p in (("bq", t.bq), ("baq", t.baq), ("mq", t.mq))})
    if os.environ.get("LFQ_PILEUP_ATOMIC"):         # the read-major kernels: a column's observations in any order
        pack = lambda d: (d["nt"].astype(np.uint32) | (d["bq"].astype(np.uint32) << 8) | (d["baq"].astype(np.uint32) << 16)
                          | (d["mq"].astype(np.uint32) << 24))
        a, b = pack(got), pack({k: h[k][:n_obs] for k in ("nt", "bq", "baq", "mq")})
        for c in range(ncols):
            assert np.array_equal(np.sort(a[int(off[c]):int(off[c + 1])]), np.sort(b[int(off[c]):int(off[c + 1])])), (ctx, c)
    else:
        for k in ("nt", "bq", "baq", "mq"):
            assert np.array_equal(got[k], h[k][:n_obs]), (ctx, k)


@pytest.mark.parametrize("name", [r.name for r in TABLE])
def test_row_on_the_device(caller, oracle, name):
    """one row: the SNV pileup in both nt layouts against the oracle, the indel pileup against the plain restatement"""
    import lofreq_amd as la
    row = BY_NAME[name]
    out = pe.oracle_out(oracle, row)
    ref = row.ref.encode()
    try:
        for packed in (True, False):
            caller.set_pileup_nt_packed(packed)
            dt = la.pileup_snv_tracks(caller, row.reads, ref, row.begin, row.end, lb=_lb(row), min_plp_bq=row.min_plp_bq)
            _check_snv(dt, packed, out, (name, "packed" if packed else "bytes"))
    finally:
        caller.set_pileup_nt_packed(True)
    cols, col_pos = la.pileup_indel_columns(caller, row.reads, ref, row.begin, row.end, min_plp_idq=row.min_plp_idq)
    gu.assert_indel_columns_equal(cols, col_pos, _indel_ref(row), row.begin, row.end)


@pytest.mark.parametrize("group", ["row", "round", "region"])
def test_rows_on_a_resident_read_set(caller, oracle, group):
    """the route of test_resident_readset_chain: one upload per row, both pileups from the read set"""
    import lofreq_amd as la
    n_ev = 0
    for row in TABLE:
        if row.group != group:
            continue
        rs = la.ReadSet(caller, row.reads, row.ref.encode())
        try:
            dt = rs.pileup_snv(row.begin, row.end, min_plp_bq=row.min_plp_bq, sync=True)
            _check_snv(dt, True, pe.oracle_out(oracle, row), (row.name, "read set"))
            cols, col_pos = rs.pileup_indels(row.begin, row.end, min_plp_idq=row.min_plp_idq)
            n_ev += gu.assert_indel_columns_equal(cols, col_pos, _indel_ref(row), row.begin, row.end)
        finally:
            rs.close()
    assert n_ev > 0
