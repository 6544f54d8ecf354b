"""CPU half of the count / scan boundary tests (tests/count_edges.py): the numpy restatement of the count kernels' outputs
against the oracle on every row, the builder against its own arrays, and the routing rule against the table's claims."""
import numpy as np
import pytest

import count_edges as ce
import dp_edges as de
import util

TABLE = ce.boundary_table()
SMALL = [r for r in TABLE if not r.checks.get("large")]

# every instantiation lfq_launch_count can launch.  (The launch macros also instantiate lfq_count_multi_kernel<true, ..>
# and lfq_count_kernel<.., false>, behind branches nothing reaches: a packed batch below count_multi_below takes the
# shallow kernel, and lazy_strand is never set together with the general path or the detection limit.)
LAUNCHABLE = [
    "lfq_count_shallow_kernel<true, 4>", "lfq_count_shallow_kernel<true, 8>", "lfq_count_shallow_kernel<true, 16>",
    "lfq_count_shallow_kernel<false, 4>", "lfq_count_shallow_kernel<false, 8>", "lfq_count_shallow_kernel<false, 16>",
    "lfq_count_multi_kernel<false, true, 4>", "lfq_count_multi_kernel<false, true, 8>", "lfq_count_multi_kernel<false, true, 16>",
    "lfq_count_multi_kernel<false, false, 4>", "lfq_count_multi_kernel<false, false, 8>", "lfq_count_multi_kernel<false, false, 16>",
    "lfq_count_lean_kernel<true>", "lfq_count_lean_kernel<false>",
    "lfq_count_fast_kernel<false, false, false>", "lfq_count_fast_kernel<false, false, true>",
    "lfq_count_fast_kernel<false, true, false>", "lfq_count_fast_kernel<false, true, true>",
    "lfq_count_fast_kernel<true, true, false>", "lfq_count_fast_kernel<true, true, true>",
    "lfq_count_kernel<false, true>", "lfq_count_kernel<true, true>",
]


def assert_ref_equals_oracle(ref, ores, host):
    """counts_ref against the oracle, field by field (the oracle has no `gated` / `coverage`: a gated column is one it left
    at zero, and its strand counts are per nucleotide)"""
    for f in ("n_err_probs", "alt_counts", "alt_raw_counts"):
        assert np.array_equal(ref[f], ores[f]), f
    assert np.array_equal(ref["tested"].astype(np.int32), ores["tested"])
    assert np.array_equal(ref["kmax"], ores["alt_counts"].max(1))
    rb = np.asarray(host["ref_base"])
    code = np.full(len(rb), -1)
    for x, ch in enumerate(b"ACGT"):
        code[rb == ch] = x
    live = np.nonzero(ref["gated"] == 0)[0]
    assert (code[live] >= 0).all()
    assert not ores["n_err_probs"][ref["gated"] != 0].any()
    rc = code[live]
    assert np.array_equal(ref["ref_fw"][live], ores["fw"][live, rc]) and np.array_equal(ref["ref_rv"][live], ores["rv"][live, rc])
    for a in range(3):
        x = np.array([[y for y in range(4) if y != r][a] for r in range(4)])[rc]
        assert np.array_equal(ref["alt_fw"][live, a], ores["fw"][live, x]), a
        assert np.array_equal(ref["alt_raw_counts"][live, a] - ref["alt_fw"][live, a], ores["rv"][live, x]), a


def _ref_conf(conf):
    return {k: v for k, v in conf.items() if k in ("min_bq", "min_alt_bq", "min_cov")}


@pytest.mark.parametrize("group", ["routing", "shallow", "lean", "scan"])
def test_counts_ref_against_oracle(oracle, group):
    """the restatement equals the oracle on every small row (rows of the general path: under the default filters, which is
    what it covers)"""
    n = 0
    for r in SMALL:
        if r.group != group:
            continue
        host = r.build()
        kw = _ref_conf(r.conf)
        ores, _ = util.run_oracle(oracle, host, **kw)
        ref = ce.counts_ref(host, kw)
        assert_ref_equals_oracle(ref, ores, host)
        lens = np.diff(host["col_off"].astype(np.int64))
        cov = host.get("coverage_plp")
        assert np.array_equal(ref["coverage"], lens if cov is None else cov), r.name
        n += int(ref["tested"].sum())
        assert ref["tested"].any() and (not ref["tested"].all() or len(ref) == 1), r.name
    assert n > 0


def test_counts_ref_against_oracle_many_columns(oracle):
    """... and on a 200 000-column cut of the many-columns batch"""
    host = ce.cut_batch(ce.many_columns_batch(), 0, ce.MANY_CUT)
    ores, _ = util.run_oracle(oracle, host)
    ref = ce.counts_ref(host)
    assert_ref_equals_oracle(ref, ores, host)
    frac = ref["tested"].mean()
    assert 0.004 < frac < 0.02, frac
    assert ores["emitted"].any(1).sum() > 0.2 * ref["tested"].sum()          # records all along the batch
    assert (ref["alt_raw_counts"].sum(1) > ref["alt_counts"].sum(1)).any()
    assert (ref["n_err_probs"] > ref["alt_counts"].max(1))[ref["tested"] != 0].all()    # no column of one alt allele only


def test_counts_ref_gates_and_thresholds():
    """the restatement on a hand-made batch: qualities either side of both thresholds, codes 4..7, the three gates"""
    nt = np.array([0, 1, 1 | 8, 1, 4, 5, 6, 7, 2, 0 | 8], np.uint8)
    bq = np.array([5, 9, 10, 5, 40, 40, 40, 40, 93, 6], np.uint8)
    one = dict(nt=nt, bq=bq, col_off=np.array([0, 10], np.uint64), ref_base=np.frombuffer(b"A", np.uint8))
    r = ce.counts_ref(one, dict(min_bq=6, min_alt_bq=10))[0]
    assert r["n_err_probs"] == 3 and list(r["alt_counts"]) == [1, 1, 0] and list(r["alt_raw_counts"]) == [3, 1, 0]
    assert list(r["alt_fw"]) == [2, 1, 0] and (r["ref_fw"], r["ref_rv"]) == (1, 1) and r["kmax"] == 1 and r["tested"] == 1
    r = ce.counts_ref(one)[0]
    assert r["n_err_probs"] == 4 and list(r["alt_counts"]) == [2, 1, 0]
    for ref, cov, nb, gated in ((b"N", 10, 10, 1), (b"a", 10, 10, 1), (b"A", 21, 10, 1), (b"A", 20, 10, 0), (b"A", 0, 0, 1)):
        h = dict(one, ref_base=np.frombuffer(ref, np.uint8), coverage_plp=np.array([cov], np.int32),
                 num_bases=np.array([nb], np.int32))
        r = ce.counts_ref(h)[0]
        assert r["gated"] == gated and r["coverage"] == cov and (r["n_err_probs"] > 0) == (not gated), (ref, cov, nb)


def test_builder_hits_lengths_residues_and_alts():
    """every row's builder produced the lengths, start residues, reference bases, alt positions and qualities it names --
    read back from the arrays"""
    seen_q, seen_codes, seen_refs = set(), set(), set()
    for r in SMALL:
        if r.group == "scan":
            continue
        host = r.build()
        off = host["col_off"].astype(np.int64)
        assert len(host["specs"]) == len(off) - 1 and len(host["index"]) <= len(off) - 1
        min_alt_bq = max(r.conf.get("min_bq", ce.MIN_BQ), r.conf.get("min_alt_bq", ce.MIN_ALT_BQ))
        ref = ce.counts_ref(host, _ref_conf(r.conf))
        for c, s in enumerate(host["specs"]):
            nt, bq = host["nt"][off[c]:off[c + 1]], host["bq"][off[c]:off[c + 1]]
            assert len(nt) == s["n"] and off[c] == s["start"], (r.name, c)
            if s["res"] is not None:
                assert off[c] % 16 == s["res"], (r.name, c)
            if s["tag"] == "filler":
                assert 1 <= s["n"] <= 15 and not ref["tested"][c]
            assert chr(host["ref_base"][c]) == s["ref"]
            seen_refs.add(s["ref"])
            code = nt & 7
            base = max("ACGT".find(s["ref"]), 0)
            alt = np.nonzero((code <= 3) & (code != base))[0]
            assert tuple(alt.tolist()) == s["alt_pos"] and tuple(code[alt].tolist()) == s["alt_code"], (r.name, c)
            if s["ref"] in "ACGT" and not ref["gated"][c]:
                others = [x for x in range(4) if x != base]
                for a in range(3):
                    sel = alt[code[alt] == others[a]]
                    assert ref["alt_raw_counts"][c, a] == len(sel)
                    assert ref["alt_counts"][c, a] == int((bq[sel] >= min_alt_bq).sum()), (r.name, c, a)
            seen_q |= set(bq[alt].tolist()) | set(bq[:: max(len(bq) // 50, 1)].tolist())
            seen_codes |= set(code.tolist())
            if s["tag"] == "deep":
                assert s["alt_pos"][-1] == s["n"] - 1
                if r.group == "routing":
                    assert s["n"] == np.diff(off).max() and (np.diff(off) == s["n"]).sum() == 1
        # chunk edges: an "edges" column has an alt base on both sides of every boundary between chunks it spans
        for c in host["index"]:
            s = host["specs"][c]
            g = s["start"] + np.array(s["alt_pos"], np.int64)
            inner = np.arange(s["start"] // 16 * 16 + 16, s["start"] + s["n"], 16)
            if len(s["alt_pos"]) > 2 and len(inner) and s["tag"] != "n_lo":
                assert np.isin(inner, g).all() and np.isin(inner - 1, g).all(), (r.name, c)
    assert {5, 6, 9, 10, 31, 32, 93} <= seen_q
    assert seen_codes == set(range(8)) and {"N", "g", "t"} <= seen_refs


def test_routing_rows_have_one_deep_column():
    for r in SMALL:
        if r.group != "routing":
            continue
        host = r.build()
        lens = np.diff(host["col_off"].astype(np.int64))
        deep = int(r.name.split("/")[1]) if r.name.split("/")[1].isdigit() else lens.max()
        assert lens.max() == deep and (lens > 64).sum() == 1 and len(lens) >= 70, r.name
        assert host["col_off"][int(np.argmax(lens))] % 16 == 15


def test_shallow_rows_geometry():
    """the lengths rows hold every length at every residue; the placement rows' special columns sit where the row says"""
    rows = {r.name: r for r in SMALL}
    for lpg in ce.LPGS:
        host = rows["shallow/lpg%d/lengths" % lpg].build()
        off = host["col_off"].astype(np.int64)
        got = {(int(off[c + 1] - off[c]), int(off[c] % 16)) for c in host["index"]}
        want = ce.shallow_lengths(lpg)
        assert {0, 1, 15, 16, 17, 31, 32, 33, 16 * ce.AHEAD * lpg - 1, 16 * ce.AHEAD * lpg, 16 * ce.AHEAD * lpg + 1} <= set(want)
        for n in want:
            for res in (0, 1, 8, 15):
                assert (n, res) in got, (lpg, n, res)
        assert np.diff(off).max() == ce.LPG_MAX_DEPTH[lpg]
        # a second round exists for every lanes-per-column setting, and the deepest column reaches the last one
        assert ce.shallow_rounds(ce.LPG_MAX_DEPTH[lpg], lpg) >= 2
        assert (ce.LPG_MAX_DEPTH[lpg] + 15 + 15) // 16 > (ce.shallow_rounds(ce.LPG_MAX_DEPTH[lpg], lpg) - 1) * ce.AHEAD * lpg
        g = 64 // lpg
        for tail in (1, 63, 64, 65):
            for kind in ("empty", "gated"):
                host = rows["shallow/lpg%d/%s/tail%d" % (lpg, kind, tail)].build()
                ref = ce.counts_ref(host)
                lens = np.diff(host["col_off"].astype(np.int64))
                ncols = len(lens)
                assert ncols == 192 + tail
                special = np.array([0, 64, 63, 127] + list(range(128 + g, 128 + 2 * g)) + list(range(ncols - tail, ncols)))
                dead = (lens == 0) if kind == "empty" else (ref["gated"] != 0)
                assert np.array_equal(np.nonzero(dead)[0], np.sort(special)), (lpg, kind, tail)
                if kind == "gated":
                    assert (lens[special] > 0).all()
                assert ref["tested"][~dead].all()
        for ncols in (1, 63, 64, 65, 255, 256, 257):
            host = rows["shallow/lpg%d/ncols%d" % (lpg, ncols)].build()
            lens = np.diff(host["col_off"].astype(np.int64))
            assert len(lens) == ncols and lens[0] == lens.max() == ce.LPG_MAX_DEPTH[lpg]
        host = rows["shallow/lpg%d/coverage_gates" % lpg].build()
        ref = ce.counts_ref(host)
        tags = {s["tag"]: c for c, s in enumerate(host["specs"])}
        assert list(np.nonzero(ref["gated"])[0]) == [10, 30, 63]
        assert not ref["gated"][tags["2nb=cov"]] and not ref["gated"][tags["nb=min_cov"]]
        assert (ref["coverage"] != np.diff(host["col_off"].astype(np.int64))).all()


def test_lean_rows_geometry():
    rows = {r.name: r for r in SMALL}
    host = rows["lean/chunks/one_thr"].build()
    off = host["col_off"].astype(np.int64)
    got = set()
    for c in host["index"][1:-2]:
        n_ch = (off[c + 1] + 15) // 16 - off[c] // 16
        last = off[c + 1] - ((off[c + 1] - 1) // 16) * 16
        got.add((int(n_ch), int(off[c] % 16), int(last)))
    for n_ch in ce.LEAN_CHUNKS:
        for res in (0, 9):
            for last in (1, 16):
                assert (n_ch, res, last if (n_ch > 1 or last > res) else res + 1) in got, (n_ch, res, last)
    assert off[1] - off[0] >= ce.MULTI_BELOW
    # low-quality kept rows in chunk 0, in the last chunk, inside the first trip and behind it
    c = [c for c in host["index"] if (off[c + 1] + 15) // 16 - off[c] // 16 == 259][0]
    bq = host["bq"][off[c]:off[c + 1]]
    low = (bq >= ce.MIN_BQ) & (bq <= ce.Q_LO)
    assert low[:16].any() and low[-16:].any() and low[16:2064].any() and low[2100:-16].any()
    for ncols in (ce.WG_WAVES - 1, ce.WG_WAVES, ce.WG_WAVES + 1):
        host = rows["lean/ncols%d" % ncols].build()
        assert len(host["col_off"]) - 1 == ncols + 1
    subset, shift = ce.C["LFQ_BOUND_SUBSET"][0], ce.C["LFQ_BOUND_SHIFT"][0]
    for inside in (63, 64):
        host = rows["lean/n_lo/%d_inside" % inside].build()
        off = host["col_off"].astype(np.int64)
        ref = ce.counts_ref(host)
        for c in host["index"]:
            bq = host["bq"][off[c]:off[c + 1]]
            first = 16 - off[c] % 16
            n_last = (off[c + 1] - 1) % 16 + 1
            low = (bq >= ce.MIN_BQ) & (bq <= ce.Q_LO)
            assert low[:first].all() and low[len(bq) - n_last:-1].all() and bq[-1] == 40
            assert low[first:first + subset].sum() == inside and low[first + subset:].sum() >= 1024
            assert (inside >> shift) == (1 if inside == 64 else 0)
            assert ref["kmax"][c] == 1 and de.dp_class(1, int(ref["n_err_probs"][c])) == "light"


def test_scan_rows_geometry():
    for r in SMALL:
        if r.group != "scan":
            continue
        host = r.build()
        ncols = len(host["ref_base"])
        ref = ce.counts_ref(host)
        tested = np.nonzero(ref["tested"])[0]
        assert list(tested) == list(host["tested"])
        want = [i for i in (0, ce.SCAN_TILE - 1, ce.SCAN_TILE, ce.SCAN_TILE + 1, ncols - 1) if i < ncols]
        assert set(want) <= set(tested.tolist())
        for i, cls in host["tested"].items():
            assert de.dp_class(int(ref["kmax"][i]), int(ref["n_err_probs"][i])) == cls
    classes = lambda side: {cls for i, cls in host["tested"].items() if side(i)}
    assert ncols == 2 * ce.SCAN_TILE + 1
    assert classes(lambda i: ce.SCAN_TILE - 3 <= i < ce.SCAN_TILE) == classes(lambda i: ce.SCAN_TILE <= i < ce.SCAN_TILE + 3) \
        == {"light", "mid", "big"}


def test_expected_kernel_and_coverage_of_instantiations():
    """expected_kernel gives the name each row claims; every launchable instantiation is claimed; each routing constant has
    a row on both sides; the tables use only constants source_constants() returned"""
    claimed = set()
    for r in TABLE:
        for name in r.consts:
            assert name in ce.C and ce.C[name][1].count(":") == 1, (r.name, name)
        if r.build is None:
            deep = ce.WRAP_DEPTH
        elif r.checks.get("large"):
            deep = ce.MANY_DEEPEST
        else:
            deep = int(np.diff(r.build()["col_off"].astype(np.int64)).max())
        same_thr = r.conf.get("min_alt_bq", ce.MIN_ALT_BQ) == r.conf.get("min_bq", ce.MIN_BQ)
        general = bool(r.conf.get("min_jq", 0) > 0 or r.conf.get("def_alt_bq", 0) == -1)
        for route, kern in r.kernels.items():
            assert route in ce.ROUTES
            got = ce.expected_kernel(deep, route.endswith("packed"), route.startswith("dense"), same_thr, general)
            assert got == kern, (r.name, route, got, kern)
            claimed.add(kern)
    assert len(LAUNCHABLE) == len(set(LAUNCHABLE)) == 22
    assert claimed == set(LAUNCHABLE), (set(LAUNCHABLE) - claimed, claimed - set(LAUNCHABLE))
    depths = {int(r.name.split("/")[1]) for r in TABLE if r.group == "routing" and r.name.split("/")[1].isdigit()}
    for const, below in (("count_lpg4_below", 0), ("count_lpg8_below", 0), ("count_multi_below", 1)):
        v = ce.C[const][0]
        assert {v - below, v - below + 1} <= depths, const
    for d in depths:
        for thr in ("one_thr", "two_thr"):
            assert any(r.name == "routing/%d/%s" % (d, thr) for r in TABLE)
    assert (ce.LPG4_BELOW, ce.LPG8_BELOW, ce.MULTI_BELOW) == (320, 900, 4096)       # the defaults the issue names
    # the large rows reach the loops they are there for
    assert ce.MANY_NCOLS > ce.C["maxdepth grid"][0][0] * ce.C["maxdepth grid"][0][1]
    assert ce.MANY_NCOLS > ce.C["shallow workgroup cap"][0] * ce.C["shallow columns per workgroup"][0]
    assert -(-ce.MANY_NCOLS // ce.SCAN_TILE) > ce.C["LFQ_SCAN_THREADS"][0]
    assert (ce.WRAP_NCOLS - 300) * ce.WRAP_DEPTH >= 2 ** 32 > (ce.WRAP_NCOLS - 301) * ce.WRAP_DEPTH
    assert ce.WRAP_DEPTH < ce.MULTI_BELOW


def test_source_constants_fail_loudly():
    with pytest.raises(AssertionError):
        ce._define("lfq_kernels.hip", "LFQ_NO_SUCH_CONSTANT")
    for name, (value, at) in ce.C.items():
        assert value is not None and ":" in at, name
