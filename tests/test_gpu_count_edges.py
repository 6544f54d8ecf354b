"""-m gpu: the count and scan kernels at their routing and chunk boundaries (tests/count_edges.py).

Every small row of the table runs on four routes, and so on the instantiation the table names for each:
  dense/byte, dense/packed   lfq_call_snvs_batch with the dense counts, host tracks in either nt layout: counts against the
                             oracle and the numpy restatement (counts_ref), records against the oracle;
  lazy/byte, lazy/packed     lfq_set_dense_strand_counts(0) + lfq_snv_batch_device on device tracks -- the only way into the
                             lean kernel: the decision counts against counts_ref, the records built from the sparse output
                             byte-identical to the dense route's.
"""
import numpy as np
import pytest

import count_edges as ce
import util
from test_gpu_parity import _compare_records

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TABLE = ce.boundary_table()
SMALL = [r for r in TABLE if not r.checks.get("large")]
SENTINEL = 0xA5


def _device_batch(la, host, packed, max_col_obs, device=0):
    """the host tracks in HBM, padded to the 16-byte contract of the track pointers"""
    import torch
    dev = torch.device("cuda", device)

    def up(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.uint8)
        t = torch.zeros((a.size + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
        if a.size:
            t[: a.size] = torch.from_numpy(a).to(dev)
        return t

    def up32(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)

    nt = util.to_pileup_batch(la, host).packed().nt if packed else host["nt"]
    off = torch.from_numpy(host["col_off"].astype(np.int64)).to(dev)
    b = la.PileupBatch(up(nt), up(host["bq"]), up(host["mq"]), off, up(host["ref_base"]), baq=up(host["baq"]), sq=up(host["sq"]),
                       coverage_plp=up32(host.get("coverage_plp")), num_bases=up32(host.get("num_bases")), on_device=True,
                       max_col_obs=max_col_obs, nt_packed=packed)
    b.ncols = len(host["col_off"]) - 1
    return b


def _layer1(la, caller, batch, conf_kw, fill=0, pvals_capacity=None, device=0):
    """lfq_snv_batch_device + lfq_batch_finish -> (dense counts, sparse records sorted by column, stats, dp_work, conf)"""
    import torch
    dev = torch.device("cuda", device)
    ncols = max(batch.ncols, 1)
    cap = pvals_capacity or ncols
    d_counts = torch.full((ncols * 64,), fill, dtype=torch.uint8, device=dev)
    d_pvals = torch.zeros(cap * 128, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    conf = la.VarcallConf(**conf_kw)
    caller.snv_batch_device(batch, conf, d_counts, d_pvals, cap)
    st = caller.batch_finish()
    work = caller.dp_work()
    counts = d_counts.cpu().numpy().view(la.COL_COUNTS_DTYPE)[: batch.ncols].copy()
    pv = d_pvals[: int(st.n_pvals) * 128].cpu().numpy().view(la.COL_PVALS_DTYPE).copy()
    del d_counts, d_pvals
    return counts, pv[np.argsort(pv["col"], kind="stable")], st, work, conf


def _ref_conf(conf):
    return {k: v for k, v in conf.items() if k in ("min_bq", "min_alt_bq", "min_cov")}


def _medians(oracle, host, ref):
    """median_ref_bq of every column under def_alt_bq = -1 (snpcaller.c:363-379; int_median through the oracle)"""
    import ctypes as C
    off = host["col_off"].astype(np.int64)
    out = np.full(len(off) - 1, -1, np.int32)
    for c in np.nonzero(ref["gated"] == 0)[0]:
        nt, bq = host["nt"][off[c]:off[c + 1]], host["bq"][off[c]:off[c + 1]]
        q = bq[(nt & 7) == b"ACGT".index(bytes([host["ref_base"][c]]))].astype(np.int32)
        if len(q):
            out[c] = oracle.lib().orc_int_median((C.c_int * len(q))(*q.tolist()), len(q))
    return out


@pytest.mark.parametrize("row", SMALL, ids=[r.name for r in SMALL])
def test_small_rows(caller, oracle, row):
    import lofreq_amd as la
    host = row.build()
    ncols = len(host["col_off"]) - 1
    deepest = int(np.diff(host["col_off"].astype(np.int64)).max())
    ores, oconf = util.run_oracle(oracle, host, **row.conf)
    ref = ce.counts_ref(host, _ref_conf(row.conf))             # (general rows: its gates and coverage still hold)
    full = not row.checks.get("general")
    n_tested = int(ores["tested"].sum())
    batch = util.to_pileup_batch(la, host)

    # ---- dense routes ----
    dense = {}
    for route, b in (("dense/byte", batch), ("dense/packed", batch.packed())):
        conf = la.VarcallConf(**row.conf)
        recs, counts, st = caller.call_snvs(b, conf, want_counts=True)
        work = caller.dp_work()
        util.assert_counts_equal(counts, ores, host)
        for f in (ce.REF_FIELDS if full else ("gated", "coverage")):
            assert np.array_equal(counts[f], ref[f]), (route, f, np.nonzero((counts[f] != ref[f]).reshape(ncols, -1).any(1))[0][:8])
        assert np.array_equal(counts["kmax"], ores["alt_counts"].max(1)), route
        if row.checks.get("median"):
            assert np.array_equal(counts["median_ref_bq"], _medians(oracle, host, ref)), route
        _compare_records(la, recs, ores, host)
        assert conf.bonf_subst == oconf.bonf_subst and conf.num_snv_tests == oconf.num_snv_tests, route
        assert st.n_tested == n_tested, route
        dense[route] = (recs, work)
    assert dense["dense/byte"][0].tobytes() == dense["dense/packed"][0].tobytes()
    recs = dense["dense/packed"][0]

    if row.checks.get("scan"):
        tested = np.nonzero(ores["tested"])[0]
        assert ores["emitted"][tested].any(1).all(), "the row is wrong: the oracle prunes a tested column"
        want = {"light": 0, "mid": 0, "big": 0}
        for cls in host["tested"].values():
            want[cls] += 1
        for _, work in dense.values():
            assert (work["n_light"], work["n_mid"], work["n_big"]) == (want["light"], want["mid"], want["big"]), work
        assert (np.diff(recs["col"]) >= 0).all() and sorted(set(recs["col"].tolist())) == tested.tolist()

    # ---- lazy routes ----
    caller.set_dense_strand_counts(False)
    try:
        for route, packed in (("lazy/byte", False), ("lazy/packed", True)):
            outs = []
            for mco in ((deepest, 0) if row.checks.get("max_col_obs_0") else (deepest,)):
                counts, pv, st, work, conf = _layer1(la, caller, _device_batch(la, host, packed, mco), row.conf)
                outs.append((counts.tobytes(), pv.tobytes(), int(st.n_tested)))
            assert all(o == outs[0] for o in outs), (route, "max_col_obs = 0 changes the result")
            for f in (ce.LAZY_FIELDS if full else ("gated", "coverage")):
                assert np.array_equal(counts[f], ref[f]), (route, f, np.nonzero((counts[f] != ref[f]).reshape(ncols, -1).any(1))[0][:8])
            for f in ("n_err_probs", "alt_counts"):
                assert np.array_equal(counts[f], ores[f]), (route, f)
            assert st.n_tested == n_tested, route
            lazy_recs = la.finalize_pvals(conf, pv, None)
            assert lazy_recs.tobytes() == recs.tobytes(), route
            if row.checks.get("scan"):
                tested = np.nonzero(ores["tested"])[0]
                assert pv["col"].tolist() == tested.tolist(), route
                assert np.array_equal(pv["bonf"], ores["bonf_used"][tested]), route
            if packed and "rows" in row.checks:
                assert work["n_light"] == n_tested == len(host["index"])
                assert (work["rows"] > 0) if row.checks["rows"] == "> 0" else (work["rows"] == 0), (row.checks["rows"], work)
            if packed and "sparse_entries" in row.checks:
                # the shallow kernel is the only one that honours lfq_set_dense_counts(0): below count_multi_below the
                # untested columns' entries keep the fill, from count_multi_below on every entry is written
                caller.set_dense_counts(False)
                try:
                    sparse, pv2, st2, _, _ = _layer1(la, caller, _device_batch(la, host, True, deepest), row.conf, fill=SENTINEL)
                finally:
                    caller.set_dense_counts(True)
                assert pv2.tobytes() == pv.tobytes() and st2.n_tested == st.n_tested
                t = counts["tested"] != 0
                assert 0 < t.sum() < ncols
                assert sparse[t].tobytes() == counts[t].tobytes()
                kept = (sparse[~t].view(np.uint8).reshape(-1, 64) == SENTINEL).all(1)
                if row.checks["sparse_entries"] == "kept":
                    assert kept.all(), "an untested column's entry was written: not the shallow kernel"
                else:
                    assert not kept.any() and sparse.tobytes() == counts.tobytes(), "an entry was left unwritten: the shallow kernel"
    finally:
        caller.set_dense_strand_counts(True)


@pytest.mark.timeout(300)
def test_many_columns(caller, oracle):
    """1024 * 4096 + 4097 columns of 1..3 observations on device tracks: lfq_maxdepth_kernel's stride loop (max_col_obs = 0),
    the shallow kernel's, the carry loop of lfq_scan_sums_kernel.  All columns' dense counts against counts_ref, every
    sparse record's Bonferroni factor against 3 x the running count of tested columns, the first 200 000 and the last
    5000 columns against the oracle."""
    import lofreq_amd as la
    host = ce.many_columns_batch()
    ncols = len(host["col_off"]) - 1
    assert ncols == ce.MANY_NCOLS and int(np.diff(host["col_off"].astype(np.int64)).argmax()) == ncols - 1
    ref = ce.counts_ref(host)
    n_tested = int(ref["tested"].sum())
    prefix = 3 * np.cumsum(ref["tested"].astype(np.int64))
    outs = []
    for mco in (ce.MANY_DEEPEST, 0):
        counts, pv, st, work, conf = _layer1(la, caller, _device_batch(la, host, True, mco), {}, pvals_capacity=n_tested + 16)
        outs.append((counts, pv, int(st.n_tested)))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes() and outs[0][2] == outs[1][2]
    for f in ce.REF_FIELDS:
        bad = np.nonzero((counts[f] != ref[f]).reshape(ncols, -1).any(1))[0]
        assert bad.size == 0, (f, bad[:8], bad.size)
    assert st.n_tested == n_tested
    assert len(pv) > 0.2 * n_tested and (np.diff(pv["col"]) > 0).all()
    assert pv["col"].max() == ncols - 1 and pv["col"].min() < ce.SCAN_TILE
    assert np.array_equal(pv["bonf"], prefix[pv["col"]])
    recs = la.finalize_pvals(conf, pv, None)
    for c0, c1 in ((0, ce.MANY_CUT), (ncols - ce.MANY_TAIL, ncols)):
        cut = ce.cut_batch(host, c0, c1)
        kw = dict(bonf_subst=int(prefix[c0 - 1])) if c0 else {}
        ores, _ = util.run_oracle(oracle, cut, **kw)
        util.assert_counts_equal(counts[c0:c1], ores, cut)
        t = np.nonzero(ores["tested"])[0]
        assert np.array_equal(ores["bonf_used"][t], prefix[c0 + t])
        r = recs[(recs["col"] >= c0) & (recs["col"] < c1)].copy()
        r["col"] -= c0
        assert len(r) > 0
        _compare_records(la, r, ores, cut)


@pytest.mark.timeout(300)
def test_beyond_2_32_observations(caller, oracle):
    """the shallow kernel on a resident batch of more than 2^32 observations (a 5 Mb genome at 1000x is one): dense counts and
    records of the 400 columns around the crossing, of every 1000th column and of every 21st planted one against the oracle"""
    import lofreq_amd as la
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    if free < 24e9:
        print("test_beyond_2_32_observations: %.1f GB of device memory free, 24 GB needed" % (free / 1e9))
        pytest.skip("less than 24 GB of device memory free")
    seed, depth, ncols, period = ce.WRAP_SEED, ce.WRAP_DEPTH, ce.WRAP_NCOLS, ce.WRAP_PERIOD
    own = la.SnvCaller(0)                               # a context of its own: 15 GB of tracks, freed with it
    batch = None
    try:
        batch = own.synth_batch(seed, depth, ncols, plant_period=period, nt_packed=True)
        conf = la.VarcallConf()
        recs, counts, st = own.call_snvs(batch, conf, want_counts=True, records_capacity=1 << 18)
    finally:
        del batch
        own.close()
        torch.cuda.empty_cache()
    assert ncols * depth > 2 ** 32
    tested = counts["tested"] != 0
    assert st.n_tested == int(tested.sum()) and conf.bonf_subst == 3 * st.n_tested       # (consistency of the device's own outputs)
    before = np.concatenate([[0], np.cumsum(tested)])                                   # tested columns in front of column c
    cross, cols = ce.wrap_columns()
    assert (cross - 1) * depth < 2 ** 32 <= cross * depth and cross + 200 <= ncols
    ranges = [(cross - 200, 400)] + [(int(c), 1) for c in cols if not cross - 200 <= c < cross + 200]
    n_recs = 0
    for c0, n in ranges:
        host = oracle.synth_fill(seed, depth, period, c0, n)
        host["sq"] = None
        kw = dict(bonf_subst=3 * int(before[c0])) if before[c0] else {}
        ores, _ = util.run_oracle(oracle, host, **kw)
        util.assert_counts_equal(counts[c0:c0 + n], ores, host)
        assert np.array_equal(counts["kmax"][c0:c0 + n], ores["alt_counts"].max(1))
        r = recs[(recs["col"] >= c0) & (recs["col"] < c0 + n)].copy()
        r["col"] -= c0
        _compare_records(la, r, ores, host)
        n_recs += len(r)
    assert n_recs > 0 and tested[cross - 200:cross + 200].any()
