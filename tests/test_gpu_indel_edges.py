"""-m gpu: the indel caller at its gate, packing and routing boundaries (tests/indel_edges.py).

Every row of the table goes through lfq_call_indels_batch on IndelColumns.from_columns (pseudo-columns packed on the host) against
the oracle, once with every test emitted and once with the default conf; the `dp route` and `flags` rows also against the exact
tail.  The rows that carry reads go through ReadSet.pileup_indels and the live columns (pseudo-columns packed by
lfq_indel_pack_kernel): the same records as the host packing, byte for byte, and the oracle's.  The gate rows on one contig give
the VCF the 2.1.4 binary wrote (tests/golden/indel_edges.json).

Indel mode exposes no name of the count kernel it launched: the `count route` rows are held to the oracle's records at the depth
the table claims (test_indel_edges.py holds max_col_obs and the kernel name to the routing rule)."""
import json

import pytest

import dp_edges as de
import indel_edges as ie
import util
from test_gpu_indel import _run_both
from test_indel_edges import EVERY_TEST, GOLDEN, assert_columns_are_the_rows, golden_conf_kwargs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TABLE = ie.table()
BY_NAME = {r.name: r for r in TABLE}
COLUMN_ROWS = [r.name for r in TABLE if r.group != "wide"]
READS_ROWS = [r.name for r in TABLE if r.reads and r.group != "wide"]
WORST = {}                                   # what the p-values were compared with -> the largest |dlog p| seen


def _classes(work):
    return {"light": work["n_light"], "mid": work["n_mid"], "big": work["n_big"]}


def _against_exact(row, recs):
    """the records of a run with every test emitted against the exact tail, with the bound of test_gpu_dp_edges.py"""
    assert len(recs) == len(row.claim["exact"])
    for r, t, levels in zip(recs, row.claim["tests"], row.claim["exact"]):
        lp = ie.exact_log_tail(t[3], levels)
        d = abs(util.log_of(r["pvalue"]) - lp)
        WORST["exact tail"] = max(WORST.get("exact tail", 0.0), d)
        assert d <= de.log_close(util.log_of(r["pvalue"]), lp, t[4]), (row.name, t, r["pvalue"], lp, d)


@pytest.mark.parametrize("name", COLUMN_ROWS)
def test_row_from_columns(caller, oracle, name):
    """one row on the host-pack route: every record field, ntests and the conf's counters against the oracle (test_gpu_indel's
    _run_both), the tested set as the table claims it, the DP classes of dp_work, the exact tail"""
    import lofreq_amd as la
    row = BY_NAME[name]
    if row.claim.get("twin"):
        # values outside a quality's range mean nothing to the reference: the records are those of the row that holds what the
        # clamps make of them (which is a row of its own, and compared with the oracle as such)
        for kw in (EVERY_TEST, {}):
            got, n = la.call_indels(caller, la.IndelColumns.from_columns(row.cols), la.VarcallConf(**dict(row.conf, **kw)))
            twin = la.IndelColumns.from_columns(BY_NAME[row.claim["twin"]].cols)
            want, n_twin = la.call_indels(caller, twin, la.VarcallConf(**dict(row.conf, **kw)))
            assert n == n_twin == len(row.claim["tests"]) and len(want) > 0
            assert got.tobytes() == want.tobytes(), "the clamped twin gives other records"
        return
    for kw in (EVERY_TEST, {}):
        cols, tests, recs = _run_both(la, caller, oracle, row.cols, **dict(row.conf, **kw))
        got = [(int(t["col"]), int(t["side"]), int(t["event"]), int(t["count"]), int(t["n_err_probs"])) for t in tests]
        assert got == row.claim["tests"]
        if "classes" in row.claim:
            assert _classes(caller.dp_work()) == row.claim["classes"], caller.dp_work()
        if kw:
            assert len(recs) == len(tests), "a p-value of 1: the row is wrong"
            assert [int(r["count"]) for r in recs] == [t[3] for t in row.claim["tests"]]
            for r, t in zip(recs, tests):
                WORST["oracle"] = max(WORST.get("oracle", 0.0), abs(util.log_of(r["pvalue"]) - util.log_of(t["pvalue"])))
            if "exact" in row.claim:
                _against_exact(row, recs)


def _records_equal_oracle(la, oracle, row, cols, col_pos, recs, ntests, conf, kw):
    """records of the live columns against the oracle's tests on the row's column dicts (columns named by position)"""
    want_cols = la.IndelColumns.from_columns(row.cols)
    oconf = oracle.default_conf(**kw)
    tests = oracle.call_indels_batch(want_cols.flat(), oconf)
    assert ntests == len(tests) and conf.bonf_indel == oconf.bonf_indel and conf.num_indel_tests == oconf.num_indel_tests
    exp = tests[tests["emitted"] == 1]
    assert len(recs) == len(exp)
    for r, t in zip(recs, exp):
        pos = int(col_pos[int(r["col"])])
        ctx = (row.name, pos, int(t["side"]), int(t["event"]))
        assert pos == row.reads["pos"][int(t["col"])] and int(r["side"]) == int(t["side"]), ctx
        key = cols.keys[int(r["side"])][int(r["event"])]
        assert key == want_cols.keys[int(t["side"])][int(t["event"])], ctx
        for k in ("qual", "dp", "sb", "ref_fw", "ref_rv", "alt_fw", "alt_rv", "hrun", "count"):
            assert int(r[k]) == int(t[k]), (ctx, k, r[k], t[k])
        assert int(r["bonf"]) == int(t["bonf_used"]) and r["af"] == t["af"], ctx
        util.assert_pvalue_close(r["pvalue"], t["pvalue"], ctx=str(ctx), n_obs=int(t["n_err_probs"]))
        WORST["oracle"] = max(WORST.get("oracle", 0.0), abs(util.log_of(r["pvalue"]) - util.log_of(t["pvalue"])))
        ref, alt = cols.ref_alt(int(r["col"]), int(r["side"]), int(r["event"]))
        assert la.format_indel_record("chr1", pos, cols, r) == oracle.format_indel("chr1", pos, ref, alt, t), ctx
    return tests


def _device_and_host_pack(la, caller, row, kw):
    """the row's reads -> resident read set -> live indel columns -> calls with the pseudo-columns packed on the device, then the
    same columns through the host packing -> (cols, col_pos, device records, ntests, conf)"""
    rd = row.reads
    rs = la.ReadSet(caller, rd["reads"], rd["ref"].encode())
    try:
        cols, col_pos = rs.pileup_indels(0, rd.get("end", len(rd["ref"])))
        assert cols._c_ptr is not None
        conf = la.VarcallConf(**kw)
        dev, ntests = la.call_indels(caller, cols, conf, records_capacity=max(64, 2 * len(row.claim["tests"])))
        cols._c_ptr = None                                      # the same data, host route
        conf_h = la.VarcallConf(**kw)
        host, ntests_h = la.call_indels(caller, cols, conf_h, records_capacity=max(64, 2 * len(row.claim["tests"])))
    finally:
        rs.close()
    assert ntests == ntests_h and conf.bonf_indel == conf_h.bonf_indel
    assert dev.tobytes() == host.tobytes(), "device packing and host packing give other records"
    return cols, col_pos, dev, ntests, conf


@pytest.mark.parametrize("name", READS_ROWS)
def test_row_from_reads(caller, oracle, name):
    """one `reads` row on the device-pack route: the live columns are the row's, the records byte-identical to the host packing
    and equal to the oracle's"""
    import lofreq_amd as la
    row = BY_NAME[name]
    for extra in (EVERY_TEST, {}):
        kw = dict(row.conf, **extra)
        cols, col_pos, recs, ntests, conf = _device_and_host_pack(la, caller, row, kw)
        assert_columns_are_the_rows(cols.flat(), col_pos, row)
        tests = _records_equal_oracle(la, oracle, row, cols, col_pos, recs, ntests, conf, kw)
        assert [(int(t["col"]), int(t["side"]), int(t["count"]), int(t["n_err_probs"])) for t in tests] == \
            [(c, sd, k, n) for c, sd, e, k, n in row.claim["tests"]]
        if extra:
            assert len(recs) == len(tests)
            if "exact" in row.claim:
                _against_exact(row, recs)


def test_state_does_not_reach_the_records(oracle):
    """the screen variant of an indel batch follows the K histogram of the context's previous one: batch A (K <= 3), B (K up to
    40), A again on one context, B on a fresh one -- A's records both times and B's on both contexts are the same bytes"""
    import lofreq_amd as la
    a, b = BY_NAME["state/A"], BY_NAME["state/B"]
    runs = {}
    for ctx, order in (("one", (a, b, a)), ("fresh", (b,))):
        own = la.SnvCaller(0)
        try:
            for i, row in enumerate(order):
                cols, tests, recs = _run_both(la, own, oracle, row.cols, **dict(row.conf, **EVERY_TEST))
                assert len(recs) == len(tests) == len(row.claim["tests"])
                assert _classes(own.dp_work()) == row.claim["classes"]
                runs[(ctx, i)] = recs.tobytes()
        finally:
            own.close()
    assert runs[("one", 0)] == runs[("one", 2)]
    assert runs[("one", 1)] == runs[("fresh", 0)]


def test_wide_region_part_boundaries(caller, oracle):
    """400 001 columns, an event in the last column of a part of the threaded column scan and in the first of the next, for 2, 3
    and 4 parts: the tests are found and their records are the oracle's"""
    import lofreq_amd as la
    row = BY_NAME["wide/part_boundaries"]
    kw = dict(row.conf, **EVERY_TEST)
    cols, col_pos, recs, ntests, conf = _device_and_host_pack(la, caller, row, kw)
    assert cols.ncols == ie.WIDE_N == len(col_pos)
    assert_columns_are_the_rows(cols.flat(), col_pos, row)
    _records_equal_oracle(la, oracle, row, cols, col_pos, recs, ntests, conf, kw)
    assert ntests == len(row.claim["tests"]) == len(recs) == conf.num_indel_tests
    assert [int(col_pos[int(r["col"])]) for r in recs] == row.reads["pos"]


def test_gate_rows_give_the_binary_vcf(caller):
    """the device chain alone -- read set, indel pileup, device packing, calls -- on the contig of the gate and poly-AT rows: the
    VCF lines and the test count of the 2.1.4 binary"""
    import lofreq_amd as la
    fx = json.load(open(GOLDEN))
    ref, reads, spans = ie.golden_contig()
    assert [list(s) for s in spans] == fx["rows"]
    rs = la.ReadSet(caller, reads, ref.encode())
    try:
        cols, col_pos = rs.pileup_indels(0, len(ref))
        assert cols._c_ptr is not None
        conf = la.VarcallConf(**golden_conf_kwargs(fx))
        recs, ntests = la.call_indels(caller, cols, conf, records_capacity=256)
    finally:
        rs.close()
    assert ntests == fx["num_indel_tests"] == conf.num_indel_tests
    lines = [la.format_indel_record("chr1", int(col_pos[int(r["col"])]), cols, r).rstrip("\n") for r in recs]
    assert lines == fx["vcf"]


def test_zz_worst_deviation():
    """prints the largest |dlog p| the tests above saw (run last in the module)"""
    print("\nindel edges: max |dlog p| against %s; bound %g up to |log p| = %g" % (
        ", ".join("the %s %.3g" % kv for kv in sorted(WORST.items())) or "nothing (tests deselected)", util.PV_LOG_TOL, util.PV_DEEP_LOG))
