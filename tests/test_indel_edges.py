"""CPU half of the indel boundary tests (tests/indel_edges.py): the table's constants are the sources' own, every claim of every
row holds against the oracle's call_indels restatement, the p-values of the `dp route` and `flags` rows against the exact tail,
the column dicts of the `reads` rows against the oracle's pileup, and the oracle against the 2.1.4 binary's VCF of the gate rows
(tests/golden/indel_edges.json)."""
import json
import os
import re

import mpmath
import numpy as np
import pytest

import count_edges as ce
import dp_edges as de
import indel_edges as ie
import util

TABLE = ie.table()
BY_NAME = {r.name: r for r in TABLE}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "indel_edges.json")
EVERY_TEST = dict(sig=1.0, bonf_dynamic=0, bonf_indel=1)      # every test is emitted (a p-value of exactly 1 aside)


def oracle_tests(oracle, row, **kw):
    from lofreq_amd.indel import IndelColumns
    cols = IndelColumns.from_columns(row.cols)
    conf = oracle.default_conf(**dict(row.conf, **kw))
    return cols, oracle.call_indels_batch(cols.flat(), conf), conf


def test_constants_are_the_sources_own():
    """the geometry of the pack kernel as its launch line has it, the routing constants through dp_edges / count_edges"""
    src = open(os.path.join(ie.pe.ROOT, ie.PLP_SRC)).read()
    m = re.search(r"hipLaunchKernelGGL\(lfq_indel_pack_kernel, dim3\(\(unsigned\)\(\(a\.n_tests \+ (\d+)\) / (\d+)\)\), dim3\((\d+)\)", src)
    assert m and int(m.group(2)) == ie.PACK_WAVES == int(m.group(1)) + 1 and int(m.group(3)) == ie.PACK_WAVES * ie.PACK_LANES
    assert ie.Q_MISSING == ie.Q_MAX + 1 and ie.POLYAT_AF == 0.05
    for name in ("LFQ_MID_K", "LFQ_BIG_K", "suspicious", "lfq_khist_thr"):
        assert de.C[name][1].split(":")[0] in ("lfq_internal.h", "lfq_kernels.hip"), name
    for name in ("count_lpg4_below", "count_lpg8_below", "count_multi_below"):
        assert ce.C[name][1].startswith("lfq_host.cpp:"), name


def test_table_is_complete():
    """the boundaries the table is there for"""
    groups = {r.group for r in TABLE}
    assert groups == {"gates", "poly-AT", "pack", "flags", "count route", "dp route", "state", "wide"}
    # pack: every pair of lengths with a tested event, on both sides; the test counts; the observation totals
    lengths = BY_NAME["pack/lengths"]
    seen = set()
    for c in lengths.cols:
        for sn in ("ins", "dels"):
            if c[sn]["events"]:
                seen.add((len(c[sn]["ne_q"]), sum(len(e["q"]) for e in c[sn]["events"])))
    assert seen == {(a, b) for a in ie.LENGTHS for b in ie.LENGTHS if b}
    assert {len(BY_NAME["pack/tests/%d" % n].claim["tests"]) for n in (1, 3, 4, 5, 8, 9)} == {1, 3, 4, 5, 8, 9}
    totals = {sum(t[4] for t in r.claim["tests"]) % 16 for r in TABLE if r.name.startswith("pack/observations/")}
    assert totals == {0, 1, 15}
    first_mid_last = [[len(e["q"]) for e in c["ins"]["events"]].index(1) for c in BY_NAME["pack/three_events"].cols]
    assert first_mid_last == [0, 1, 2]
    assert {r.conf["flag"] for r in TABLE if r.group == "flags"} == {0, 2, 4, 8, 14}
    # count route: the deepest pseudo-column on each side of the three constants, with and without the sq track in use
    depths = {(r.claim["max_col_obs"], bool(r.conf["flag"] & ie.USE_SQ)) for r in TABLE if r.group == "count route"}
    assert depths == {(n + d, sq) for n in (ce.LPG4_BELOW, ce.LPG8_BELOW, ce.MULTI_BELOW - 1) for d in (0, 1) for sq in (False, True)}
    lpgs = {r.claim["kernel"] for r in TABLE if r.group == "count route"}
    assert lpgs == {"lfq_count_multi_kernel<false, true, 4>", "lfq_count_multi_kernel<false, true, 8>",
                    "lfq_count_multi_kernel<false, true, 16>", "lfq_count_fast_kernel<false, true, true>"}
    # dp route: both classes at every light / mid / big boundary, and MAXK - 1, MAXK, MAXK + 1 of every screen variant
    b = ie.dp_boundaries()
    by = {}
    for boundary, k, n, cls in b:
        by.setdefault(boundary, set()).add(cls)
    assert by["suspicious at MID_K - 1"] == by["suspicious floor"] == by["suspicious above the floor"] == {"light", "mid"}
    assert {cls for bd, k, n, cls in b if k in (de.BIG_K - 1, de.BIG_K)} == {"mid", "big"}
    light_ks = {k for bd, k, n, cls in b if cls == "light"}
    for maxk in de.SCREEN_MAXK:
        assert {maxk - 1, maxk, maxk + 1} <= light_ks, maxk
    for boundary, k, n, cls in b:                       # the smallest depth of the class: one row less is another class, or no row
        assert cls != "light" or n == k + 1 or de.dp_class(k, n - 1) != "light", (boundary, k, n)
    assert BY_NAME["state/A"].claim["kmax"] <= 3 and BY_NAME["state/B"].claim["kmax"] == 40
    wide = BY_NAME["wide/part_boundaries"]
    assert wide.reads["pos"] == sorted({ie.WIDE_N * p // parts - d for parts in (2, 3, 4) for p in range(1, parts) for d in (0, 1)})
    assert ie.WIDE_N == 400001 and len(wide.cols) == len(wide.reads["pos"]) == 10


def test_polyat_line_in_float_and_double():
    """the rows on the line: count / denom equals the float 0.05f, and lies below it once the division is done in double"""
    for name in ("line/5_of_100", "line/1_of_20", "line/50_of_1000", "tails/105_5", "tails/85_5"):
        c = BY_NAME["poly-AT/" + name].cols[0]
        cnt, denom = len(c["ins"]["events"][0]["q"]), c["coverage_plp"] - c["num_tails"]
        assert np.float32(cnt) / np.float32(denom) == np.float32(0.05) and cnt / denom < float(np.float32(0.05))
        assert len(BY_NAME["poly-AT/" + name].claim["tests"]) == 2
    c = BY_NAME["poly-AT/tails/105_5"].cols[0]
    assert (c["coverage_plp"], c["num_tails"]) == (105, 5)
    c = BY_NAME["poly-AT/tails/104_5"].cols[0]
    assert (c["coverage_plp"], c["num_tails"]) == (104, 5)
    c = BY_NAME["gates/min_cov/coverage_above_sum_below"].cols[0]
    assert c["coverage_plp"] >= ie.MIN_COV > c["num_non_indels"] + 4 + 3
    c = BY_NAME["gates/min_cov/coverage_below_sum_equal"].cols[0]
    assert c["coverage_plp"] < ie.MIN_COV == c["num_non_indels"] + 4 + 3


def _claimed(tests):
    return [(int(x["col"]), int(x["side"]), int(x["event"]), int(x["count"]), int(x["n_err_probs"])) for x in tests]


def test_claims_against_the_oracle(oracle):
    """the tested set, every test's count and n_err_probs, the Bonferroni factor used: with every test emitted, and with the
    default dynamic factor (1 + the tests so far, lofreq_call.c:693-696)"""
    for row in TABLE:
        cols, tests, conf = oracle_tests(oracle, row, **EVERY_TEST)
        assert _claimed(tests) == row.claim["tests"], row.name
        assert (tests["bonf_used"] == 1).all() and conf.num_indel_tests == len(tests) and conf.bonf_indel == 1, row.name
        assert row.claim.get("twin") or np.isfinite(tests["logp"]).all(), row.name      # (a twin's row is out of range on purpose)
        cols, tests, conf = oracle_tests(oracle, row)
        assert _claimed(tests) == row.claim["tests"], row.name
        assert tests["bonf_used"].tolist() == list(range(2, 2 + len(tests))), row.name
        assert conf.bonf_indel == 1 + len(tests), row.name
        if "max_col_obs" in row.claim:
            assert max(t[4] for t in row.claim["tests"]) == row.claim["max_col_obs"] == int(tests["n_err_probs"].max())
        if "classes" in row.claim:
            got = {"light": 0, "mid": 0, "big": 0}
            for x in tests:
                got[de.dp_class(int(x["count"]), int(x["n_err_probs"]))] += 1
            assert got == row.claim["classes"], row.name


def test_byte_clamps_twin(oracle):
    """the twin of the out-of-range row holds the clamped values and nothing else differs; its p-values are finite"""
    raw, twin = BY_NAME["pack/bytes/raw"], BY_NAME[BY_NAME["pack/bytes/raw"].claim["twin"]]
    clamp = lambda v: min(max(v, 0), ie.Q_MAX)
    clamp8 = lambda v: -1 if v < 0 else min(v, ie.Q_MAX)
    n_out = 0
    for a, b in zip(raw.cols, twin.cols):
        for sn in ("ins", "dels"):
            assert [clamp(v) for v in a[sn]["ne_q"]] == b[sn]["ne_q"] and [clamp8(v) for v in a[sn]["ne_mq"]] == b[sn]["ne_mq"]
            for x, y in zip(a[sn]["events"], b[sn]["events"]):
                assert [clamp(v) for v in x["q"]] == y["q"]
                for k in ("aq", "mq", "sq"):
                    assert [clamp8(v) for v in x[k]] == y[k]
                    n_out += sum(v != w for v, w in zip(x[k], y[k]))
                n_out += sum(v != w for v, w in zip(x["q"], y["q"]))
            n_out += sum(v != w for v, w in zip(a[sn]["ne_q"], b[sn]["ne_q"]))
    assert n_out >= 20
    vals = lambda key: {v for c in raw.cols for sn in ("ins", "dels") for e in c[sn]["events"] for v in e[key]}
    assert {-5, 254, 255, 300} <= vals("q") | {v for c in raw.cols for v in c["ins"]["ne_q"]}
    assert 0 in {v for c in raw.cols for v in c["ins"]["ne_q"]}
    for key in ("aq", "mq", "sq"):
        assert {-1, 0, 254, 300} <= vals(key), key
    assert 255 in vals("aq") and 255 in vals("sq")
    m = BY_NAME["pack/bytes/mq255"].cols[0]
    assert 255 in m["ins"]["ne_mq"] and 255 in m["ins"]["events"][0]["mq"] and 255 in m["dels"]["events"][0]["mq"]


def test_exact_tail_levels():
    """dp_edges.exact_tail with the body's probability and further levels given: the same sum as the two-quality form, and a
    direct convolution of three levels"""
    with mpmath.workdps(de.DPS):
        two = de.exact_tail(5, dict(n=300, q=20, q2=10, n_q2=3))
        same = de.exact_tail(5, dict(n=300, p=de.lut_p(20), levels=[(3, de.lut_p(10))]))
        assert abs(two / same - 1) < mpmath.mpf(10) ** -50
        pa, pb, pc = mpmath.mpf("0.01"), mpmath.mpf("0.3"), mpmath.mpf("0.8")
        pmf = [mpmath.mpf(1)]
        for n, p in ((20, pa), (4, pb), (3, pc)):
            for _ in range(n):
                pmf = [(pmf[j] if j < len(pmf) else 0) * (1 - p) + (pmf[j - 1] * p if j else 0) for j in range(len(pmf) + 1)]
        for k in (1, 3, 6):
            direct = mpmath.fsum(pmf[k:])
            got = de.exact_tail(k, dict(n=27, p=pa, levels=[(4, pb), (3, pc)]))
            assert abs(got / direct - 1) < mpmath.mpf(10) ** -50, k
        # the merged probability: one quality alone is its LUT value; two multiply as independent errors
        assert ie.merged_p(-1, -1, -1, 30) == mpmath.mpf(de.lut_p(30))
        assert abs(ie.merged_p(-1, -1, 10, 20) - (1 - (1 - mpmath.mpf(de.lut_p(10))) * (1 - mpmath.mpf(de.lut_p(20))))) < mpmath.mpf(10) ** -55
        assert ie.merged_p(-1, 0, -1, 93) > ie.MQ0_P


EXACT_ROWS = [r.name for r in TABLE if "exact" in r.claim]


def test_oracle_against_the_exact_tail(oracle):
    """dp route and flags: the oracle's log p within the bound of test_dp_edges.py (dp_edges.log_close) of the 60-digit tail of
    the pseudo-column's levels; a dp route row's p-value is finite, no sentinel and within util.PV_DEEP_LOG"""
    worst = {}
    for name in EXACT_ROWS:
        row = BY_NAME[name]
        cols, tests, _ = oracle_tests(oracle, row, **EVERY_TEST)
        assert len(tests) == len(row.claim["exact"]) > 0
        for x, levels in zip(tests, row.claim["exact"]):
            assert sum(n for n, _ in levels) == x["n_err_probs"], name
            lp_ref = float(x["logp"])
            if row.group == "dp route":
                assert np.isfinite(lp_ref) and abs(lp_ref) <= util.PV_DEEP_LOG, (name, lp_ref)
                assert x["pvalue"] not in (util.LDBL_MAX, util.LDBL_MIN) and 0 < x["pvalue"] < 1, (name, x["pvalue"])
            lp = ie.exact_log_tail(int(x["count"]), levels)
            d = abs(lp_ref - lp)
            assert d <= de.log_close(lp_ref, lp, int(x["n_err_probs"])), (name, lp_ref, lp, d)
            worst[row.group] = max(worst.get(row.group, 0.0), d)
    print("oracle vs exact tail: max |dlog p| %s (bound %g)" % (worst, util.PV_LOG_TOL))


def test_flags_rows_would_show_a_leak():
    """the alignment quality on the reads of all three insertions instead of the tested one's moves the exact tail by orders of
    magnitude more than the bound"""
    levels = BY_NAME["flags/columns/flag8"].claim["exact"][0]
    plain, mine = (-1, -1, -1, ie.FLAGS_Q), (-1, -1, ie.FLAGS_AQ, ie.FLAGS_Q)
    assert sorted(levels) == [(3, mine), (45, plain)]
    leaked = [(9, mine), (39, plain)]
    assert abs(ie.exact_log_tail(3, leaked) - ie.exact_log_tail(3, levels)) > 1e8 * util.PV_LOG_TOL


# ---- the reads of the `reads` rows give the row's columns -------------------------------------------------------------------------

def flat_column(flat, keys, c):
    """column c of flat indel arrays (IndelColumns.flat() / the oracle's pileup) as a plain dict"""
    d = {k: int(flat[k][c]) for k in ("coverage_plp", "num_tails", "num_non_indels", "num_ins", "num_dels", "hrun")}
    d["ref"] = chr(int(flat["ref_base"][c]))
    for sd, sn in enumerate(("ins", "dels")):
        a, b = int(flat["ne_off"][sd][c]), int(flat["ne_off"][sd][c + 1])
        e0, e1 = int(flat["ev_off"][sd][c]), int(flat["ev_off"][sd][c + 1])
        events = []
        for e in range(e0, e1):
            r0, r1 = int(flat["rd_off"][sd][e]), int(flat["rd_off"][sd][e + 1])
            events.append({"key": keys[sd][e], "fw": int(flat["ev_fw"][sd][e]), "rv": int(flat["ev_rv"][sd][e]),
                           **{k: flat["rd_" + k][sd][r0:r1].tolist() for k in ("q", "aq", "mq", "sq")}})
        d[sn] = {"non_fw": int(flat["non_fw"][sd][c]), "non_rv": int(flat["non_rv"][sd][c]), "ne_q": flat["ne_q"][sd][a:b].tolist(),
                 "ne_mq": flat["ne_mq"][sd][a:b].tolist(), "events": events}
    return d


def flat_keys(flat):
    out = []
    for sd in range(2):
        kc, off = bytes(flat["key_chars"][sd]), flat["key_off"][sd]
        out.append([kc[int(off[e]):int(off[e + 1])].decode() for e in range(len(off) - 1)])
    return out


def assert_columns_are_the_rows(flat, col_pos, row):
    """the columns of `flat` at the row's positions are the row's dicts; no other column has an event"""
    from lofreq_amd.indel import IndelColumns
    want = IndelColumns.from_columns(row.cols)
    wflat, keys = want.flat(), flat_keys(flat)
    at = {int(p): c for c, p in enumerate(col_pos)}
    for i, p in enumerate(row.reads["pos"]):
        assert flat_column(flat, keys, at[p]) == flat_column(wflat, want.keys, i), (row.name, p)
    others = np.ones(len(col_pos), bool)
    others[[at[p] for p in row.reads["pos"]]] = False
    for sd in range(2):
        assert (np.diff(flat["ev_off"][sd])[others] == 0).all(), row.name
    return at


READS_ROWS = [r.name for r in TABLE if r.reads]


def test_reads_rows_exist():
    groups = {BY_NAME[n].group for n in READS_ROWS}
    assert groups == {"gates", "poly-AT", "pack", "flags", "wide"}
    assert "pack/lengths" in READS_ROWS and "poly-AT/ignored_A_beside_AT" in READS_ROWS


@pytest.mark.parametrize("name", READS_ROWS)
def test_reads_give_the_columns(oracle, name):
    row = BY_NAME[name]
    rd = row.reads
    P = oracle.pack_reads(rd["reads"], rd["ref"].encode())
    out = oracle.pileup_region(P, 0, rd.get("end", len(rd["ref"])))
    assert_columns_are_the_rows(out["flat"], out["col_pos"], row)
    if row.group == "wide":
        assert len(out["col_pos"]) == ie.WIDE_N


# ---- the binary as witness for the gates ------------------------------------------------------------------------------------------

def golden_conf_kwargs(fx):
    import golden_util as gu
    args = list(fx["call_args"])
    i = args.index("-C")
    min_cov = int(args[i + 1])
    del args[i:i + 2]
    kw, no_default_filter = gu.conf_kwargs(args)
    assert no_default_filter and kw["bonf_dynamic"] == 0
    kw.pop("bonf_subst")
    return dict(kw, min_cov=min_cov, bonf_indel=1)


def test_oracle_against_the_binary(oracle):
    """the gate and poly-AT rows on one contig: the oracle's pileup and calls give the VCF lines and the test count the 2.1.4
    binary wrote, and per row the tests the table claims"""
    fx = json.load(open(GOLDEN))
    ref, reads, spans = ie.golden_contig()
    assert [list(s) for s in spans] == fx["rows"] and len(ref) == fx["contig_len"] and len(reads) == fx["n_reads"]
    out = oracle.pileup_region(oracle.pack_reads(reads, ref.encode()), 0, len(ref))
    conf = oracle.default_conf(**golden_conf_kwargs(fx))
    assert conf.min_cov == ie.MIN_COV
    tests = oracle.call_indels_batch(out["flat"], conf)
    keys = flat_keys(out["flat"])
    lines, per_row = [], {}
    for x in tests:
        pos = int(out["col_pos"][int(x["col"])])
        name = next(n for n, a, b in spans if a <= pos < b)
        per_row[name] = per_row.get(name, 0) + 1
        if x["emitted"]:
            r, key = ref[pos], keys[int(x["side"])][int(x["event"])]
            ref_alt = (r, r + key) if x["side"] == 0 else (r + key, r)
            lines.append(oracle.format_indel("chr1", pos, ref_alt[0], ref_alt[1], x).rstrip("\n"))
    assert len(tests) == fx["num_indel_tests"] == conf.num_indel_tests
    assert lines == fx["vcf"]
    for row in ie.golden_rows():
        assert per_row.get(row.name, 0) == len(row.claim["tests"]), row.name
    assert len(fx["vcf"]) == fx["num_indel_tests"] > 20          # sig = 1: every test wrote its line
