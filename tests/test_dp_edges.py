"""CPU half of the DP boundary tests (tests/dp_edges.py): the boundary table's columns hit their K and depth exactly, and the
oracle's p-values of uniform columns agree with the exact binomial tail."""
import numpy as np
import pytest

import dp_edges as de
import util


def test_table_cites_the_sources():
    """every table row names a constant that was read from the line it cites, and every boundary kind is present"""
    t = de.boundary_table()
    for e in t:
        assert e.const in de.C and e.at == de.C[e.const][1], e
        assert e.cls == de.dp_class(e.k, e.n), e
    consts = {e.const for e in t}
    for c in ("LFQ_MID_K", "LFQ_BIG_K", "suspicious", "lfq_khist_thr", "lfq_seg_class", "LFQ_SPLIT_MAX_K", "fold K",
              "combine KMAX", "big C=2 below", "LFQ_HEAVY_WAVES", "LFQ_PHASE1_CHUNKS", "LFQ_SEG_MIN_CHUNKS_SHORT",
              "LFQ_SEG_SHORT_BELOW"):
        assert c in consts, c
    ks = {e.k for e in t if e.const == "lfq_khist_thr"}
    for maxk in de.SCREEN_MAXK:
        assert {maxk - 1, maxk, maxk + 1} <= ks, maxk
    assert {"light-screen", "light-wave", "mid", "big-split", "big-unsplit"} <= {e.route for e in t}
    assert {"light", "mid", "big"} == {e.cls for e in t}


def test_builder_options():
    """alt placement, the second quality level and interleaved low-BQ rows"""
    c = de.edge_column(100, (3, 2, 1), q=30, alt_at="last", q2=20, n_q2=4, low_bq_every=9, low_bq_tail=2)
    kept = c["bq"] >= de.MIN_BQ
    assert kept.sum() == 100 and len(c["nt"]) == 100 + 99 // 9 + 2
    code = c["nt"][kept] & 7
    assert list(code[-6:]) == [1, 1, 1, 2, 2, 3] and (code[:-6] == 0).all()
    assert (c["bq"][kept] == 20).sum() == 4 and (c["bq"][kept][-6:] == 30).all()
    assert (c["bq"][~kept] < de.MIN_BQ).all() and not kept[-1] and not kept[-2]
    s = de.edge_column(50, (5, 0, 0), ref=b"G", alt_at="spread")
    assert list(np.nonzero((s["nt"] & 7) != 2)[0]) == [0, 10, 20, 30, 40] and ((s["nt"] & 7)[[0, 10]] == 0).all()


def test_table_columns_hit_k_and_depth(oracle):
    """through the oracle (default filters): n_err_probs and the largest filtered alt count exactly as the table says"""
    t = de.boundary_table()
    host = de.batch_of([de.table_column(e) for e in t])
    ores, _ = util.run_oracle(oracle, host)
    for i, e in enumerate(t):
        assert ores["n_err_probs"][i] == e.n, (e.boundary, ores["n_err_probs"][i])
        assert ores["alt_counts"][i].max() == e.k, (e.boundary, ores["alt_counts"][i])
        assert de.dp_class(int(ores["alt_counts"][i].max()), int(ores["n_err_probs"][i])) == e.cls


def _cmp_exact(ores, host, nmin=1):
    worst, n = 0.0, 0
    for c, spec in enumerate(host["specs"]):
        for a in range(3):
            k = spec["counts"][a]
            if k == 0:
                continue
            lp_ref = float(ores["logp"][c, a])
            lp = de.exact_log_tail(k, spec)
            d = abs(lp_ref - lp)
            tol = de.log_close(lp_ref, lp, spec["n"])
            assert d <= tol, (c, a, spec, lp_ref, lp, d)
            worst, n = max(worst, d), n + 1
    assert n >= nmin
    return worst


def test_oracle_against_exact_tail_table(oracle):
    """every table column, unpruned (sig = 1, bonferroni 1): the oracle's log p within util.assert_pvalue_close's bound of
    the 60-digit binomial tail"""
    t = de.boundary_table()
    host = de.batch_of([de.table_column(e) for e in t])
    ores, _ = util.run_oracle(oracle, host, sig=1.0, bonf_dynamic=0, bonf_subst=1)
    worst = _cmp_exact(ores, host, len(t))
    print("oracle vs exact tail, table: max |dlog p| %.3g" % worst)


@pytest.mark.parametrize("n,counts,q,q2,n_q2", [
    (1000, (5, 0, 0), 30, None, 0), (30000, (63, 0, 0), 30, None, 0), (30000, (64, 0, 0), 30, None, 0),
    (5000, (250, 0, 0), 20, None, 0), (4000, (9, 0, 0), 30, None, 0), (400, (7, 7, 1), 25, None, 0),
    (2000, (1, 0, 12), 30, 12, 3), (3000, (40, 39, 0), 17, 35, 7), (600, (300, 0, 0), 6, 40, 2),
])
def test_oracle_against_exact_tail_shapes(oracle, n, counts, q, q2, n_q2):
    """multi-allele columns and a second quality level on a few rows"""
    host = de.batch_of([de.edge_column(n, counts, q=q, q2=q2, n_q2=n_q2, alt_at="spread")])
    ores, _ = util.run_oracle(oracle, host, sig=1.0, bonf_dynamic=0, bonf_subst=1)
    assert ores["n_err_probs"][0] == n and tuple(ores["alt_counts"][0]) == counts
    _cmp_exact(ores, host)


def test_exact_tail_sums():
    """the exact tail against closed forms: P(X >= 0) = 1, P(X >= n) = p^n, P(X >= 1) = 1 - (1 - p)^n, and both summation
    directions of _binom_tail meet at the mean"""
    import mpmath
    with mpmath.workdps(de.DPS):
        p = mpmath.mpf(de.lut_p(20))
        spec = dict(n=300, q=20)
        assert de.exact_tail(0, spec) == 1
        assert abs(de.exact_tail(300, spec) / p ** 300 - 1) < mpmath.mpf(10) ** -50
        assert abs(de.exact_tail(1, spec) / (1 - (1 - p) ** 300) - 1) < mpmath.mpf(10) ** -50
        for k in (2, 3, 4, 5):           # mean 3: both branches
            direct = mpmath.fsum(mpmath.binomial(300, j) * p ** j * (1 - p) ** (300 - j) for j in range(k, 301))
            assert abs(de.exact_tail(k, spec) / direct - 1) < mpmath.mpf(10) ** -50, k
        two = dict(n=300, q=20, q2=10, n_q2=3)
        p2 = mpmath.mpf(de.lut_p(10))
        direct = mpmath.mpf(0)
        for j in range(4):
            direct += mpmath.binomial(3, j) * p2 ** j * (1 - p2) ** (3 - j) * de._binom_tail(5 - j, 297, de.lut_p(20))
        assert abs(de.exact_tail(5, two) / direct - 1) < mpmath.mpf(10) ** -50


def test_knife_edges_against_oracle(oracle):
    """the knife-edge batches of every route: the oracle calls exactly the columns whose exact p * bonf is below sig, and
    its p-values agree with the exact tail"""
    for kb in de.knife_batches():
        host = de.batch_of(kb["cols"])
        ores, oconf = util.run_oracle(oracle, host, **kb["conf"])
        assert oconf.bonf_subst == kb["bonf"]
        got = [bool(ores["emitted"][c].any()) for c in range(len(kb["cols"]))]
        assert got == kb["emit"], (kb["route"], kb["name"], got)
        for c, col in enumerate(kb["cols"]):
            if kb["emit"][c]:
                lp = de.exact_log_tail(col["spec"]["counts"][0], col["spec"])
                assert abs(float(ores["logp"][c, 0]) - lp) <= util.PV_LOG_TOL, (kb["route"], kb["name"])
