"""-m gpu: the bound gate in front of the screen kernel's DP (lofreq_amd/csrc/lfq_bound.h) on columns built for its edges.

Batches are packed, a few dozen columns, the deepest 4100-4300 rows deep, so that the lean count kernel -- the only one that
produces the gate's statistic n_lo -- runs when no dense counts are asked for.  Every batch is checked twice against the
oracle, each time on a fresh context run twice (the screen variant of a batch follows the context's previous batch):
  - with dense counts, as tests/test_gpu_dp_edges.py::_check_run does: counts bit-exact, records, exact tails (that call
    takes the count kernel with strand counts: no statistic, the gate inert);
  - without (what the benchmark and lfq_call_vars run): the lean kernel and the gate; records, exact tails, work counters.
Whether the gate fired shows in dp_work()["rows"]: a gated column is dropped before a row of it is read.

The statistic looks at the whole 16-observation chunks of the first trip of the count loop: the 128 chunks behind the
column's (possibly ragged) first one, i.e. column rows 16 - off0 % 16 .. 2063 - off0 % 16 at the least; rows 32..1055 lie
inside it and rows from 2080 on behind it whatever the alignment."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dp_edges as de
import util
from test_gpu_parity import _compare_records

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNE_LIB = os.path.join(ROOT, "lofreq_amd", "liblofreq_amd_tune.so")
Q_HI, Q_LOW, Q_LO = 40, 20, 31
N_LOW = 1024
INSIDE, BEHIND = 32, 2080


def _column(n, k, low=(), q_low=Q_LOW, code_low=None, q=Q_HI):
    """n rows at quality q, the k alt rows last (behind the subset); rows `low` (reference rows) get quality q_low, or base
    code code_low"""
    col = de.edge_column(n, (k, 0, 0), q=q, alt_at="last")
    low = np.asarray(low, np.int64)
    assert low.size == 0 or low.max() < n - k
    spec = dict(col["spec"])
    if code_low is not None:
        col["nt"][low] = (col["nt"][low] & 8) | code_low
        spec["n"] = n - low.size
    elif q_low < de.MIN_BQ:
        col["bq"][low] = q_low
        spec["n"] = n - low.size
    elif low.size:
        col["bq"][low] = q_low
        spec.update(q2=q_low, n_q2=int(low.size))
    col["spec"] = spec
    return col


def _batch(low_at=INSIDE, n_low=N_LOW, ncols=24, **kw):
    """ncols light columns of 4200.. rows (their starts at every alignment), K = 1..3, n_low low rows from row low_at on"""
    return de.batch_of([_column(4200 + 3 * c, 1 + c % 3, np.arange(low_at, low_at + n_low), **kw) for c in range(ncols)])


def _run(la, caller, host, kw, ores, oconf, lean, worst=None):
    conf = la.VarcallConf(**kw)
    recs, counts, st = caller.call_snvs(util.to_pileup_batch(la, host).packed(), conf, want_counts=not lean)
    work = caller.dp_work()
    if counts is not None:
        util.assert_counts_equal(counts, ores, host)
    assert conf.bonf_subst == oconf.bonf_subst
    assert st.n_tested == int(ores["tested"].sum())
    _compare_records(la, recs, ores, host)
    for r in recs:
        c = int(r["col"])
        a = [int(x) for x in ores["alt_base"][c]].index(r["alt"][0])
        spec = host["specs"][c]
        lp = de.exact_log_tail(spec["counts"][a], spec)
        d = abs(util.log_of(r["pvalue"]) - lp)
        if worst is not None:
            worst.append(d)
        assert d <= de.log_close(util.log_of(r["pvalue"]), lp, spec["n"]), (c, a, r["pvalue"], lp, d)
    n_light = sum(de.dp_class(max(s["counts"]), s["n"]) == "light" for s in host["specs"])
    assert work["n_light"] == n_light and work["n_light"] + work["n_mid"] + work["n_big"] == st.n_tested, work
    return recs, work, st


def _both(oracle, host, kw=None, runs=2):
    """-> (records, dp_work, stats) of the last lean run"""
    import lofreq_amd as la
    kw = kw or {}
    ores, oconf = util.run_oracle(oracle, host, **kw)
    out = None
    for lean in (False, True):
        caller = la.SnvCaller(0)
        try:
            for _ in range(runs):
                out = _run(la, caller, host, kw, ores, oconf, lean)
        finally:
            caller.close()
    return out + (ores,)


def test_gate_fires(oracle):
    """every column light and prunable, 1024 reference rows of Q20 inside the subset: nothing is read by a DP kernel"""
    host = _batch()
    recs, work, st, _ = _both(oracle, host)
    ncols = len(host["specs"])
    assert len(recs) == 0
    assert work["n_light"] == st.n_tested == ncols
    assert work["n_light_retry"] == 0
    assert work["rows"] == 0, work


@pytest.mark.parametrize("how", ["behind", "q_lo_plus_1", "below_min_bq", "code_n", "ragged_first_chunk"])
def test_gate_does_not_fire(oracle, how):
    """the same columns changed one way at a time so that the statistic must not see the low rows: the screen's DP runs"""
    if how == "behind":
        host = _batch(low_at=BEHIND)
    elif how == "q_lo_plus_1":
        host = _batch(q_low=Q_LO + 1)
    elif how == "below_min_bq":
        host = _batch(q_low=de.MIN_BQ - 1)
    elif how == "code_n":
        host = _batch(code_low=4)
    else:
        # 63 low rows inside the subset -- one short of the 64 the statistic is rounded down to -- and the rows of the
        # first chunk, which one lane counts under a byte mask (columns of 4203 rows: the starts 0, 11, 6, .. mod 16 leave
        # first chunks of 16, 5, 10, .. rows)
        cols = []
        for c in range(24):
            first = 16 - (4203 * c) % 16
            low = np.concatenate([np.arange(first), np.arange(INSIDE, INSIDE + 63)])
            cols.append(_column(4203, 1, low))
        host = de.batch_of(cols)
        assert any(int(o) % 16 for o in host["col_off"][:-1])
    recs, work, st, _ = _both(oracle, host)
    assert work["n_light"] == st.n_tested == len(host["specs"])
    assert work["rows"] > 0, work


def test_knife_edge_with_full_statistic(oracle):
    """columns of Q31 rows throughout (n_lo = 2048, the most the statistic can say) whose exact p * bonf falls either side
    of sig: N rows is called, N + 1 is not, on both runs of a context"""
    k, n = 15, 4200
    assert de.dp_class(k, n) == "light" and de.dp_class(k, n + 1) == "light"
    a, b = _column(n, k, q=Q_LO), _column(n + 1, k, q=Q_LO)
    bonf = de._bonf_between(de.exact_tail(k, a["spec"]), de.exact_tail(k, b["spec"]))
    for cols, emit in (([a, b], [True, False]), ([b, a], [False, True])):
        host = de.batch_of(cols)
        recs, work, st, _ = _both(oracle, host, dict(bonf_dynamic=0, bonf_subst=bonf))
        assert [any(int(r["col"]) == c for r in recs) for c in range(2)] == emit, (emit, recs)
        assert work["rows"] > 0


def test_bonferroni_dependence(oracle):
    """a column (K = 2, 64 counted rows) whose bound passes the threshold at a Bonferroni factor of 90 but not at 3: as the
    first tested column of a dynamic-Bonferroni batch its DP runs, as the last one and with a carry-in from an earlier batch
    it is gated; the columns between are gated at any factor"""
    x = lambda: _column(4200, 2, np.arange(INSIDE, INSIDE + 64))
    fill = [_column(4200 + c, 1, np.arange(INSIDE, INSIDE + N_LOW)) for c in range(28)]
    _, alone, _, _ = _both(oracle, de.batch_of([x()]))
    assert alone["rows"] > 0
    _, first_last, _, _ = _both(oracle, de.batch_of([x()] + fill + [x()]))
    assert first_last["rows"] == alone["rows"], (first_last, alone)
    _, last, _, _ = _both(oracle, de.batch_of(fill + [x()]))
    assert last["rows"] == 0, last
    _, carried, _, _ = _both(oracle, de.batch_of([x()]), dict(bonf_subst=3 * 29))
    assert carried["rows"] == 0, carried


def test_two_thresholds(oracle):
    """min_alt_bq != min_bq (the count kernel's instantiation with two thresholds): low rows that pass both are counted,
    reference rows of a quality between the two are kept rows but not counted ones"""
    kw = dict(min_alt_bq=10)
    _, work, _, _ = _both(oracle, _batch(), kw)
    assert work["rows"] == 0, work
    _, work, _, _ = _both(oracle, _batch(q_low=8), kw)
    assert work["rows"] > 0, work


def test_mixed_depths(oracle):
    """one 4200-row column among columns of 1, 17, 300 and 2049 rows, all with low rows from the start: the count loop of
    the shallow ones does not run or runs a partial first trip, their statistic is 0 or what the lanes that ran saw"""
    cols = []
    for rep in range(3):
        for n in (1, 17, 300, 2049, 4200):
            cols.append(_column(n, 1, np.arange(min(n - 1, N_LOW + 2 * INSIDE)), q=30))
    host = de.batch_of(cols)
    recs, work, st, _ = _both(oracle, host)
    assert work["n_light"] == st.n_tested == len(cols)
    assert work["rows"] > 0


@pytest.mark.parametrize("kw", [dict(def_alt_bq=-1), dict(min_jq=1)], ids=["def_alt_bq", "min_jq"])
def test_gate_inert_outside_lb(oracle, kw):
    """configurations in which an alt base does not keep its quality or a merged-quality filter applies: no gate"""
    _, work, _, _ = _both(oracle, _batch(), kw)
    assert work["rows"] > 0, work


_PROBE = r"""
import sys
sys.path.insert(0, "tests")
import numpy as np
import lofreq_amd as la
import util
import test_gpu_bound_gate as t
caller = la.SnvCaller(0)
cols = [t._column(4200 + 3 * c, 1 + c % 3, np.arange(t.INSIDE, t.INSIDE + t.N_LOW)) for c in range(12)]
cols += [t._column(4200, 3), t._column(4300, 7)]        # no low rows: one pruned by the DP, one called
host = t.de.batch_of(cols)
for want in (True, False):
    recs, counts, st = caller.call_snvs(util.to_pileup_batch(la, host).packed(), la.VarcallConf(), want_counts=want)
    w = caller.dp_work()
    print("OUT", want, recs.tobytes().hex(), counts.tobytes().hex() if want else "-", st.n_tested, w["n_light"], w["n_light_retry"])
    print("ROWS", want, w["rows"])
caller.close()
"""


def test_switch_in_the_tuning_build():
    """LFQ_BOUND_GATE=0 exists in the tuning build only and changes no result: records, counts and class sizes identical
    to the default, only the rows the DP kernels read differ; the release library does not read the variable"""
    out = {}
    for name, lib, gate in (("tune", TUNE_LIB, None), ("tune_off", TUNE_LIB, "0"), ("release_off", None, "0")):
        env = dict(os.environ)
        env.pop("LFQ_AMD_LIB", None)
        env.pop("LFQ_BOUND_GATE", None)
        if lib:
            env["LFQ_AMD_LIB"] = lib
        if gate:
            env["LFQ_BOUND_GATE"] = gate
        p = subprocess.run([sys.executable, "-c", _PROBE], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, p.stderr[-1500:]
        lines = p.stdout.splitlines()
        out[name] = ([l for l in lines if l.startswith("OUT")], [int(l.split()[2]) for l in lines if l.startswith("ROWS")])
    assert out["tune"][0] == out["tune_off"][0] == out["release_off"][0]
    assert len(out["tune"][0]) == 2 and len(out["tune"][1]) == 2
    # (rows of the two calls of a process: with dense counts -- no statistic --, then without)
    assert out["tune"][1][0] == out["tune_off"][1][0] > 0, out
    assert out["tune_off"][1][1] > out["tune"][1][1] > 0, out
    assert out["release_off"][1] == out["tune"][1], out
