"""-m gpu: the bound gate decided in the scan (lfq_scan_gate_kernel, lofreq_amd/csrc/lfq_kernels.hip) -- a light column
the gate drops gets no list entry, and the screen and retry kernels see a list of survivors.

Every batch holds a few columns of 4200 rows, so that the lean count kernel -- the one that leaves the gate's statistic --
runs; the rest is shallow to keep the oracle cheap.  What "shallow" can be where a column is to be GATED is set by the
statistic itself: lane l of the count kernel's wavefront looks at chunks 1 + l and 65 + l of the column and only if the
column has more than 66 + l interior chunks (lfq_count_column_lean's peeled first trip), so a column below 67 chunks --
1060 rows -- carries no statistic at all and is never gated.  Columns to be gated are therefore 1200 rows of Q20 (about ten
lanes, 320 counted rows); columns that must survive, mid, big and untested columns are 100-400 rows.

Expected survivors do not come from the library: `_expected` restates the statistic from the batch's bytes, takes K and the
tested prefix from the column specs and the oracle, the screen variant from the rule of lfq_call_snvs_collect, and asks
lfq_bound_check.cpp (host compiler, as tests/test_scan_gate.py) for the decision.

Every case
  - runs on a fresh context twice (the second batch's screen variant follows the first one's K histogram) against the
    oracle: records, exact tails, n_tested, class sizes (test_gpu_bound_gate._run); after each run the listed-light counter
    (lfq_debug_counters) equals the expected survivors and dp_work()["n_light"] the class size;
  - is run once more by a subprocess with the tuning build under LFQ_SCAN_GATE=0 -- three scan launches, the gate in the screen
    kernel, the parent's way: records, n_tested, n_light, n_mid, n_big, n_light_retry, n_approx_pruned, rows and cells of both
    runs are identical."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dp_edges as de
import util
from test_bound_gate import QLO, SHIFT, CODES, _compile, _run as _ask
from test_gpu_bound_gate import INSIDE, N_LOW, TUNE_LIB, _column, _run
from test_gpu_parity import _compare_records

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = de._define("lfq_kernels.hip", "LFQ_SCAN_THREADS")[0] * de._define("lfq_kernels.hip", "LFQ_SCAN_ITEMS")[0]
CNT_LIGHT = de._define("lfq_internal.h", "LFQ_CNT_LIGHT")[0]
CNT_LIST_LIGHT = de._define("lfq_internal.h", "LFQ_CNT_LIST_LIGHT")[0]
SIG_S = de.SIG * (1.0 + de.C["prune_slack"][0])
N_GATED = 1200


# ---- columns -----------------------------------------------------------------------------------------------------------

_cache = {}


def _col(kind, k=1):
    """one column of a kind; built once (batch_of copies the bytes)"""
    key = (kind, k)
    if key not in _cache:
        if kind == "gated":             # every reference row Q20: whatever the lanes of the first trip look at is counted
            c = _column(N_GATED, k, np.arange(N_GATED - k))
        elif kind == "deep_gated":      # 4200 rows, 1024 Q20 rows inside the subset
            c = _column(4200, k, np.arange(INSIDE, INSIDE + N_LOW))
        elif kind == "deep":            # 4200 rows of Q40: no statistic
            c = _column(4200, k)
        elif kind == "keep":            # shallow and Q40: no statistic, the screen's DP decides
            c = _column(120 + 10 * k, k)
        elif kind == "mid":
            c = _column(300, de.MID_K)
        elif kind == "big":
            c = _column(400, de.BIG_K)
        elif kind == "untested":
            c = _column(100, 0)
        elif kind == "x":               # test_gpu_bound_gate.test_bonferroni_dependence: dropped at a factor of 90, not at 3
            c = _column(4200, 2, np.arange(INSIDE, INSIDE + 64))
        else:
            raise ValueError(kind)
        s = c["spec"]
        want = {"mid": "mid", "big": "big", "untested": None}.get(kind, "light")
        assert de.dp_class(max(s["counts"]), s["n"]) == want, (kind, k, s)
        _cache[key] = c
    return _cache[key]


def _three_tiles():
    """2 TILE + 37 columns: gated and surviving light columns, mid, big and untested columns interleaved; survivors at tile 0's
    last column and tile 2's first, every light column of tile 1 gated"""
    cols = []
    for c in range(2 * TILE + 37):
        tile = c // TILE
        if c in (5, 2 * TILE + 20):
            cols.append(_col("deep_gated", 1 + c % 3))
        elif c in (TILE - 1, TILE - 2, 2 * TILE, 2 * TILE + 1):
            cols.append(_col("keep", 1 + c % 2))
        elif c % 509 == 7:
            cols.append(_col("mid"))
        elif c % 1021 == 11:
            cols.append(_col("big"))
        elif c % 5 == 3:
            cols.append(_col("untested"))
        elif tile != 1 and c % 7 == 2:
            cols.append(_col("keep", 1 + c % 3))
        else:
            cols.append(_col("gated", 1 + c % 2))
    return de.batch_of(cols), {}


def _no_light_tile():
    """tile 0 without a light column, tile 1 ending on a survivor, tile 2 (five columns) starting with one"""
    cols = []
    for c in range(2 * TILE + 5):
        if c < TILE:
            cols.append(_col("mid") if c % 701 == 3 else _col("big") if c % 1499 == 5 else _col("untested"))
        elif c in (2 * TILE - 1, 2 * TILE):
            cols.append(_col("keep", 2))
        elif c == TILE + 9:
            cols.append(_col("deep_gated", 2))
        elif c % 3 == 0:
            cols.append(_col("untested"))
        elif c % 11 == 4:
            cols.append(_col("keep", 1))
        else:
            cols.append(_col("gated", 1 + c % 2))
    return de.batch_of(cols), {}


def _all_gated():
    cols = [_col("deep_gated", 1 + c % 3) for c in range(20)] + [_col("gated", 1 + c % 2) for c in range(30)]
    cols += [_col("mid"), _col("big"), _col("mid")]
    return de.batch_of(cols), {}


def _none_gated():
    cols = [_col("deep", 1 + c % 3) for c in range(12)] + [_col("keep", 1 + c % 3) for c in range(30)] + [_col("mid"), _col("big")]
    return de.batch_of(cols), {}


def _bonf_tiles():
    """x() first (factor 3: its DP runs) and again in tile 2 behind 2 TILE tested columns (gated)"""
    cols = [_col("x")] + [_col("keep", 1) for _ in range(2 * TILE)] + [_col("x"), _col("keep", 1)]
    return de.batch_of(cols), {}


def _bonf_carry():
    return de.batch_of([_col("x")]), dict(bonf_subst=3 * 29)


def _k_above_maxk():
    """a context's first batch launches the variant with MAXK = 7: K = 8..12 is not decided in the scan, whatever its statistic
    (here the largest there is: 2100 Q20 rows from the column's start, at the benchmark's Bonferroni factor, with which the
    variant of the second batch, MAXK = 15, drops them)"""
    cols = [_column(4200, k, np.arange(2100)) for k in (8, 9, 10, 11, 12)] + [_col("deep_gated", k) for k in (1, 2, 3, 7)]
    cols += [_col("gated", k) for k in (1, 2)]
    return de.batch_of(cols), dict(bonf_subst=3000000)


def _inert(kw):
    def build():
        cols = [_col("deep_gated", 1 + c % 3) for c in range(8)] + [_col("gated", 1 + c % 2) for c in range(8)]
        return de.batch_of(cols + [_col("keep", 1), _col("mid"), _col("big")]), kw
    return build


CASES = {
    "three_tiles": _three_tiles, "no_light_tile": _no_light_tile, "all_gated": _all_gated, "none_gated": _none_gated,
    "bonf_tiles": _bonf_tiles, "bonf_carry": _bonf_carry, "k_above_maxk": _k_above_maxk,
    "inert_min_jq": _inert(dict(min_jq=1)), "inert_def_alt_bq": _inert(dict(def_alt_bq=-1)),
    "inert_approx": _inert(dict(approx_threshold_n=500)), "inert_dense": _inert({}),
}
DENSE = ("inert_dense",)                # cases run with dense counts asked for: no lean kernel


# ---- what the gate must decide -------------------------------------------------------------------------------------------

def _codes(host):
    """lfq_bound_code of the statistic lfq_count_column_lean leaves for every column"""
    off = host["col_off"].astype(np.int64)
    code = host["nt"] & 7
    counted = ((code <= 3) & (host["bq"] >= de.MIN_BQ) & (host["bq"] <= QLO)).astype(np.int64)
    csum = np.concatenate([[0], np.cumsum(counted)])
    out = []
    for c in range(len(off) - 1):
        cbeg = off[c] >> 4
        n_in = int(((off[c + 1] + 15) >> 4) - cbeg) - 1
        n_lo = 0
        for lane in range(max(0, min(64, n_in - 65))):
            for ch in (1 + lane, 65 + lane):
                g = int(cbeg + ch) * 16
                n_lo += int(csum[g + 16] - csum[g])
        out.append(min(n_lo >> SHIFT, CODES - 1))
    return out


def _kreg_after(ks):
    """the screen variant lfq_call_snvs_collect picks for the context's next batch from the light columns' K (0: none fits)"""
    n = len(ks)
    if n == 0:
        return None
    for thr in de.SCREEN_MAXK:
        if sum(k <= thr for k in ks) >= n - n // 2000:
            return thr + 1
    return 0


@pytest.fixture(scope="module")
def decide(tmp_path_factory):
    exe, r = _compile(tmp_path_factory.mktemp("gpu_scan_gate"), "lfq_bound_check", [])
    assert r.returncode == 0, r.stderr
    p = float(de.lut_p(QLO)).hex()

    def f(rows):                        # [(code, K, maxk, factor)] -> [dropped]
        if not rows:
            return []
        out = _ask(exe, ["D %s %d %d %d %s %s" % (p, c, k, mk, float(b).hex(), float(SIG_S).hex()) for c, k, mk, b in rows])
        return [o == "1" for o in out]
    return f


def _expected(host, kw, ores, decide):
    """-> per run of a fresh context (two): the set of light columns the scan drops, and the light columns"""
    specs = host["specs"]
    light = [c for c, s in enumerate(specs) if de.dp_class(max(s["counts"]), s["n"]) == "light"]
    assert all(bool(ores["tested"][c]) for c in light)
    prefix = np.cumsum(np.asarray(ores["tested"]).astype(np.int64))
    base = kw.get("bonf_subst", 1)
    codes = _codes(host)
    ks = [max(specs[c]["counts"]) for c in light]
    runs, kreg = [], 8                  # a context without a previous batch: lfq_screen_kreg(0)
    for _ in range(2):
        if kreg == 0:
            runs.append(set())          # the one-column-per-wavefront kernel: nothing is decided in the scan
        else:
            fac = [(0 if base == 1 else base) + 3 * int(prefix[c]) if kw.get("bonf_dynamic", 1) else base for c in light]
            d = decide([(codes[c], k, kreg - 1, float(b)) for c, k, b in zip(light, ks, fac)])
            runs.append({c for c, x in zip(light, d) if x})
        nxt = _kreg_after(ks)
        kreg = kreg if nxt is None else nxt
    return runs, light


# ---- running -------------------------------------------------------------------------------------------------------------

def _counters(caller):
    buf = (ctypes.c_int32 * 64)()
    assert caller.L.lfq_debug_counters(caller.h, buf) == 0
    return list(buf)


def _digest(recs, st, work):
    keys = ("n_light", "n_mid", "n_big", "n_light_retry", "n_approx_pruned", "rows", "cells")
    return "RUN %s %d %s" % (recs.tobytes().hex() or "-", st.n_tested, " ".join("%s=%d" % (k, work[k]) for k in keys))


def _two_runs(la, name, check=None):
    """the case on a fresh context, twice -> digests; check(run, recs, work, st, counters) after each"""
    host, kw = CASES[name]()
    caller = la.SnvCaller(0)
    out = []
    try:
        for run in range(2):
            if check:
                recs, work, st, cnt = check(caller, host, kw, run)
            else:
                conf = la.VarcallConf(**kw)
                recs, _, st = caller.call_snvs(util.to_pileup_batch(la, host).packed(), conf, want_counts=name in DENSE)
                work = caller.dp_work()
            out.append(_digest(recs, st, work))
    finally:
        caller.close()
    return out


def _probe_main(names):
    import lofreq_amd as la
    for name in names:
        for line in _two_runs(la, name):
            print(name, line)


def _switched_off(names):
    """{case: digests} from the tuning build under LFQ_SCAN_GATE=0"""
    env = dict(os.environ, LFQ_AMD_LIB=TUNE_LIB, LFQ_SCAN_GATE="0")
    code = "import sys; sys.path.insert(0, 'tests'); import test_gpu_scan_gate as t; t._probe_main(%r)" % (list(names),)
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-1500:]
    out = {}
    for l in p.stdout.splitlines():
        if " RUN " in l:
            out.setdefault(l.split()[0], []).append(l.split(" ", 1)[1])
    return out


def _case(oracle, decide, names, listed_is_class=False):
    """-> {case: (expected drops per run, light columns, dp_work per run)}"""
    import lofreq_amd as la
    off = _switched_off(names)
    res = {}
    for name in names:
        host, kw = CASES[name]()
        ores, oconf = util.run_oracle(oracle, host, **kw)
        drops, light = _expected(host, kw, ores, decide)
        works = []

        def check(caller, host, kw, run):
            if kw.get("approx_threshold_n"):        # (the Poisson gate takes columns off the list: no class sizes by the specs)
                conf = la.VarcallConf(**kw)
                recs, _, st = caller.call_snvs(util.to_pileup_batch(la, host).packed(), conf)
                work = caller.dp_work()
                assert st.n_tested == int(ores["tested"].sum()) and conf.bonf_subst == oconf.bonf_subst
                _compare_records(la, recs, ores, host)
                cnt = _counters(caller)
                assert cnt[CNT_LIGHT] == work["n_light"]
            else:
                recs, work, st = _run(la, caller, host, kw, ores, oconf, lean=name not in DENSE)
                cnt = _counters(caller)
                assert cnt[CNT_LIGHT] == work["n_light"] == len(light)
            want = cnt[CNT_LIGHT] if listed_is_class else len(light) - len(drops[run])
            print("%s run %d: light %d, listed %d (expected %d), retried %d, rows %d" % (
                name, run, cnt[CNT_LIGHT], cnt[CNT_LIST_LIGHT], want, work["n_light_retry"], work["rows"]))
            assert cnt[CNT_LIST_LIGHT] == want, (name, run, cnt[CNT_LIST_LIGHT], want)
            works.append(work)
            return recs, work, st, cnt
        mine = _two_runs(la, name, check)
        assert mine == off[name], (name, [m[-160:] for m in mine], [o[-160:] for o in off[name]])
        res[name] = (drops, light, works)
    return res


def test_three_scan_tiles(oracle, decide):
    res = _case(oracle, decide, ["three_tiles", "no_light_tile"])
    drops, light, _ = res["three_tiles"]
    for d in drops:
        kept = set(light) - d
        assert {TILE - 1, 2 * TILE} <= kept and 5 in d and 2 * TILE + 20 in d
        assert not any(TILE <= c < 2 * TILE for c in kept) and any(TILE <= c < 2 * TILE for c in d)
        assert any(c < TILE for c in d) and len(kept) > 100
    drops, light, _ = res["no_light_tile"]
    assert min(light) >= TILE
    for d in drops:
        assert {2 * TILE - 1, 2 * TILE} <= set(light) - d and TILE + 9 in d


def test_everything_and_nothing_gated(oracle, decide):
    res = _case(oracle, decide, ["all_gated", "none_gated"])
    drops, light, works = res["all_gated"]
    assert all(d == set(light) for d in drops)              # an empty light part in front of the mid and big entries
    assert all(w["n_mid"] == 2 and w["n_big"] == 1 and w["n_light_retry"] == 0 for w in works)
    drops, light, works = res["none_gated"]
    assert all(not d for d in drops) and all(w["rows"] > 0 for w in works)


def test_bonferroni_dependence_across_tiles(oracle, decide):
    res = _case(oracle, decide, ["bonf_tiles", "bonf_carry"])
    drops, light, _ = res["bonf_tiles"]
    assert all(d == {2 * TILE + 1} for d in drops), drops    # the same column: kept as the first tested one, dropped in tile 2
    drops, light, works = res["bonf_carry"]
    assert all(d == {0} for d in drops) and all(w["rows"] == 0 for w in works)


def test_k_above_maxk_is_retried_not_dropped(oracle, decide):
    res = _case(oracle, decide, ["k_above_maxk"])
    drops, light, works = res["k_above_maxk"]
    host, _ = CASES["k_above_maxk"]()
    wide = {c for c in light if max(host["specs"][c]["counts"]) > 7}
    assert len(wide) == 5 and drops[0] == set(light) - wide
    assert works[0]["n_light_retry"] == len(wide)           # (equal to the switched-off run's: _case)
    assert drops[1] == set(light)                           # the second batch launches a variant that holds them


def test_inert_configurations(oracle, decide):
    """no bound gate (filters outside the LB form), the -t path, no lean kernel: three scan launches, every light column listed"""
    _case(oracle, decide, ["inert_min_jq", "inert_def_alt_bq", "inert_approx", "inert_dense"], listed_is_class=True)
