"""-m gpu: the DP kernels at their K, depth and pruning boundaries (tests/dp_edges.py).  Every case runs on a fresh context
(the screen variant of a batch follows the context's previous batch), against the oracle and, for the p-values, against
the exact binomial tail of the uniform columns."""
import os

import pytest

import dp_edges as de
import util
from test_gpu_parity import _compare_records

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

# (next to) nothing pruned.  Not sig = 1: a column whose K lies far below its mean has p = 1 - 1e-13 or so, and whether
# p * 1 < 1 then is a rounding question (the unsplit big kernel returns log p = 0 for the oracle's -9.9e-14, well within
# the 1e-10 bar; test_gpu_parity.py::test_all_pvalues_no_pruning skips such columns)
NO_PRUNE = dict(sig=0.999, bonf_dynamic=0, bonf_subst=1)


def _fresh(la, gate=None):
    c = la.SnvCaller(0)
    if gate:
        c.set_batch_gate(gate)
    return c


def _check_run(la, caller, host, kw, ores, oconf, routes, worst):
    """one call_snvs of `host` on `caller`: counts, records, exact tails (worst: route -> max |dlog p| so far);
    -> (recs, dp_work, stats)"""
    conf = la.VarcallConf(**kw)
    recs, counts, st = caller.call_snvs(util.to_pileup_batch(la, host), conf, want_counts=True)
    work = caller.dp_work()
    util.assert_counts_equal(counts, ores, host)
    assert conf.bonf_subst == oconf.bonf_subst
    assert st.n_tested == int(ores["tested"].sum())
    _compare_records(la, recs, ores, host)
    cache = {}
    for r in recs:
        c = int(r["col"])
        a = [int(x) for x in ores["alt_base"][c]].index(r["alt"][0])
        spec = host["specs"][c]
        k = spec["counts"][a]
        key = (k, spec["n"], spec["q"], spec.get("q2"), spec.get("n_q2", 0))
        if key not in cache:
            cache[key] = de.exact_log_tail(k, spec)
        lp = cache[key]
        d = abs(util.log_of(r["pvalue"]) - lp)
        route = routes[c]
        worst[route] = max(worst.get(route, 0.0), d)
        assert d <= de.log_close(util.log_of(r["pvalue"]), lp, spec["n"]), (route, c, a, r["pvalue"], lp, d)
    return recs, work, st


def _class_counts(host):
    n = {"light": 0, "mid": 0, "big": 0}
    for s in host["specs"]:
        cls = de.dp_class(max(s["counts"]), s["n"])
        if cls:
            n[cls] += 1
    return n


def _route_batches():
    """the table's columns in three batches (by depth, so that each stays small), with multi-allele shapes of the rows
    deep enough for them"""
    t = de.boundary_table()
    out = []
    for lo, hi in ((0, 3000), (3000, 8000), (8000, 10 ** 9)):
        cols, routes = [], []
        for e in t:
            if not lo <= e.n < hi:
                continue
            shapes = [None] + [s for s in de.multi_shapes(e.k) if sum(s) <= e.n and e.k <= 300]
            for s in shapes:
                cols.append(de.table_column(e, s))
                routes.append(e.route)
        out.append((de.batch_of(cols), routes))
    return out


@pytest.mark.parametrize("gate", [None, "none"])
@pytest.mark.parametrize("setting", ["no_prune", "default"])
def test_route_parity(oracle, gate, setting):
    """every table column on the route its K and depth select: counts bit-exact, records as the oracle's, p-values within
    1e-10 in log p of the exact tail, the class sizes of dp_work as the routing rule says.  Each batch runs twice on one
    context: the first run on the default screen variant, the second on the variant (or the wave kernel) its own K
    histogram selects."""
    import lofreq_amd as la
    kw = NO_PRUNE if setting == "no_prune" else {}
    worst = {}
    for host, routes in _route_batches():
        ores, oconf = util.run_oracle(oracle, host, **kw)
        exp = _class_counts(host)
        caller = _fresh(la, gate)
        try:
            for _ in range(2):
                recs, work, st = _check_run(la, caller, host, kw, ores, oconf, routes, worst)
                assert (work["n_light"], work["n_mid"], work["n_big"]) == (exp["light"], exp["mid"], exp["big"]), (work, exp)
                assert work["n_light"] + work["n_mid"] + work["n_big"] == st.n_tested
            if setting == "no_prune":
                assert len(recs) > 0
        finally:
            caller.close()
    print("\nroute parity (%s, gate %s): max |dlog p| against the exact tail per route: %s" % (
        setting, gate, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


def test_table_row_classes(oracle):
    """each table row on its own (one column per batch): the class dp_work reports is the one the table derives"""
    import lofreq_amd as la
    caller = _fresh(la)
    seen = []
    try:
        for e in de.boundary_table():
            host = de.batch_of([de.table_column(e)])
            ores, oconf = util.run_oracle(oracle, host, **NO_PRUNE)
            recs, work, st = _check_run(la, caller, host, NO_PRUNE, ores, oconf, [e.route], {})
            got = [c for c in ("light", "mid", "big") if work["n_" + c]]
            seen.append("%-70s K=%-5d N=%-6d -> %s" % (e.boundary, e.k, e.n, ",".join(got)))
            assert got == [e.cls] and st.n_tested == 1, (e, work)
    finally:
        caller.close()
    print("\n" + "\n".join(seen))


def _light_cols(ks, n, q):
    return [de.edge_column(n, (k, 0, 0), q=q, alt_at="spread") for k in ks]


@pytest.mark.parametrize("lb", [True, False], ids=["LB", "exact"])
@pytest.mark.parametrize("f", range(len(de.SCREEN_MAXK)))
def test_screen_variant(oracle, f, lb):
    """every screen-kernel width in both forms: a context primed with light columns of K <= MAXK runs the variant with
    KREG = MAXK + 1 next; of a target batch at K = MAXK - 1, MAXK, MAXK + 1 the column above MAXK and the significant
    columns go to the retry kernel, the quick exits (quality 6) do not"""
    import lofreq_amd as la
    maxk = de.SCREEN_MAXK[f]
    kw = {} if lb else (dict(def_alt_bq=-1) if f % 2 else dict(min_jq=1))
    n = max(de.light_min_n(maxk + 1), 4 * maxk)
    prime = de.batch_of(_light_cols([maxk, max(1, maxk - 3), 1], n, 6))
    target = de.batch_of(_light_cols([maxk - 1, maxk, maxk + 1, maxk - 1, maxk + 1], n, 6)
                         + [de.edge_column(n, (maxk, 0, 0), q=30, alt_at="first")])
    caller = _fresh(la)
    try:
        for host in (prime, target):
            ores, oconf = util.run_oracle(oracle, host, **kw)
            recs, work, st = _check_run(la, caller, host, kw, ores, oconf, ["light-screen"] * 6, {})
            assert work["n_light"] == len(host["specs"]) == st.n_tested
        above = sum(max(s["counts"]) > maxk for s in target["specs"])
        called = sum(bool(ores["emitted"][c].any()) and max(s["counts"]) <= maxk for c, s in enumerate(target["specs"]))
        assert called == 1 and above == 2
        lo, hi = above + called, work["n_light"]
        assert 0 < lo <= work["n_light_retry"] <= hi, (work, lo, hi)
        if "LFQ_SCREEN_ROUNDS" not in os.environ:
            assert work["n_light_retry"] == lo, (work, lo)      # the quick exits were pruned by the screen
    finally:
        caller.close()


@pytest.mark.parametrize("route", [r[0] for r in de.KNIFE_ROUTES])
def test_knife_edges(oracle, route):
    """pairs of columns whose exact p * bonf falls either side of sig (N vs N + 1 rows, a second quality level on three
    rows), and single columns at p * bonf / sig = 1 -/+ 5e-7 (inside the pruning slack): the called set is the exact one,
    the oracle's, on both runs of a context"""
    import lofreq_amd as la
    worst = {}
    for kb in de.knife_batches():
        if kb["route"] != route:
            continue
        host = de.batch_of(kb["cols"])
        ores, oconf = util.run_oracle(oracle, host, **kb["conf"])
        exp = _class_counts(host)
        caller = _fresh(la)
        try:
            for _ in range(2):
                recs, work, st = _check_run(la, caller, host, kb["conf"], ores, oconf, [route] * len(kb["cols"]), worst)
                called = [any(int(r["col"]) == c for r in recs) for c in range(len(kb["cols"]))]
                assert called == kb["emit"], (route, kb["name"], called, kb["bonf"])
                assert (work["n_light"], work["n_mid"], work["n_big"]) == (exp["light"], exp["mid"], exp["big"]), (work, exp)
        finally:
            caller.close()
    assert route in worst                   # the called columns were compared
    print("\nknife edges %s: max |dlog p| against the exact tail %.3g" % (route, worst[route]))
