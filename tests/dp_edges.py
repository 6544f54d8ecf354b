"""Columns at the routing, depth and pruning boundaries of the Poisson-binomial tail (the DP kernels of lfq_dp.hip).

Three pieces, used by test_dp_edges.py (CPU: builder and oracle against the exact tail) and test_gpu_dp_edges.py (every
route against the oracle and the exact tail):

  edge_column     a column with exact (k0, k1, k2) filtered alt counts and exactly n kept rows, every kept row with the
                  same error probability (or a second quality level on a few reference rows), optionally with rows below
                  min_bq interleaved and the alt rows first, last or spread out;
  boundary_table  every boundary of the routing rule, with the source constant, where it sits, the (K, N) on each side and
                  the class the column must take -- the constants are read from the sources, not restated;
  exact_tail      P(X >= k) for such a column, summed term by term in 60-digit arithmetic (mpmath), from the double the
                  quality LUT holds for the error probability.
"""
import os
import re
from collections import namedtuple

import mpmath
import numpy as np

import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")

MIN_BQ = 6              # lfq_conf_init's min_bq / min_alt_bq (a row below it is not a kept row)
SIG = float(np.float32(0.01))       # the conf's sig is a float; the emit and prune tests compare in double


# ---- the constants, read from the sources ----------------------------------------------------------------------------

def _find(fname, pattern):
    """(match, 'file:line') of the first line of lofreq_amd/csrc/<fname> that matches `pattern`"""
    with open(os.path.join(CSRC, fname)) as f:
        for i, line in enumerate(f, 1):
            m = re.search(pattern, line)
            if m:
                return m, "%s:%d" % (fname, i)
    raise AssertionError("%s: no line matches %r" % (fname, pattern))


def _define(fname, name):
    m, at = _find(fname, r"^#define\s+%s\s+(\d+)\b" % name)
    return int(m.group(1)), at


def source_constants():
    """{name: (value, 'file:line')} of every constant the routing rule and the split plan use"""
    c = {}
    for name in ("LFQ_MID_K", "LFQ_BIG_K", "LFQ_SPLIT_MAX_K", "LFQ_SEG_MIN_CHUNKS", "LFQ_SEG_MIN_CHUNKS_SHORT",
                 "LFQ_SEG_SHORT_BELOW", "LFQ_PHASE1_CHUNKS", "LFQ_SEG_MAX"):
        c[name] = _define("lfq_internal.h", name)
    c["LFQ_HEAVY_WAVES"] = _define("lfq_dp.hip", "LFQ_HEAVY_WAVES")
    # the suspicious rule: max(FLOOR, n_err_probs / DIV + ADD) (lfq_count_kernel and its variants)
    m, at = _find("lfq_kernels.hip", r"suspicious = max\((\d+), r\.n_err_probs / (\d+) \+ (\d+)\)")
    c["suspicious"] = (tuple(int(x) for x in m.groups()), at)
    # the screen variants: lfq_khist_thr(f) = MAXK of the variant with KREG = MAXK + 1 cells
    m, at = _find("lfq_internal.h", r"return f == 0 \? (\d+) : f == 1 \? (\d+) : f == 2 \? (\d+) : f == 3 \? (\d+) : "
                                    r"f == 4 \? (\d+) : f == 5 \? (\d+) : (\d+);")
    c["lfq_khist_thr"] = (tuple(int(x) for x in m.groups()), at)
    # the cells-per-lane classes of a row segment
    m, at = _find("lfq_dp.hip", r"return K <= (\d+) \? 0 : \(K <= (\d+) \? 1 : \(K <= (\d+) \? 2 : \(K <= (\d+) \? 3 : 4\)\)\);")
    c["lfq_seg_class"] = (tuple(int(x) for x in m.groups()), at)
    m, at = _find("lfq_dp.hip", r"constexpr int KMAX = MODE \? (\d+) : (\d+);")
    c["combine KMAX"] = ((int(m.group(2)), int(m.group(1))), at)
    m, at = _find("lfq_dp.hip", r"if \(K <= (\d+)\) \{")
    c["fold K"] = (int(m.group(1)), at)
    m, at = _find("lfq_dp.hip", r"if \(kp < (\d+) \* NW - 1\) \{")
    c["big C=2 below"] = (int(m.group(1)) * c["LFQ_HEAVY_WAVES"][0] - 1, at)
    m, at = _find("lfq_api.hip", r"P->prune_slack = ([0-9.e+-]+);")
    c["prune_slack"] = (float(m.group(1)), at)
    m, at = _find("lfq_api.hip", r"const double p = pow\(10\.0, -1\.0 \* q / 10\.0\);")
    c["quality LUT"] = (None, at)
    return c


C = source_constants()
MID_K, BIG_K, SPLIT_MAX_K = C["LFQ_MID_K"][0], C["LFQ_BIG_K"][0], C["LFQ_SPLIT_MAX_K"][0]
SUSP_FLOOR, SUSP_DIV, SUSP_ADD = C["suspicious"][0]
SCREEN_MAXK = C["lfq_khist_thr"][0]
SEG_CLASS_MAXK = C["lfq_seg_class"][0]
PHASE1 = C["LFQ_PHASE1_CHUNKS"][0]


def dp_class(kmax, n_kept):
    """the class the count kernel gives a column (lfq_kernels.hip, `suspicious`): None = not tested"""
    if kmax <= 0:
        return None
    if kmax >= BIG_K:
        return "big"
    if kmax >= MID_K or kmax >= max(SUSP_FLOOR, n_kept // SUSP_DIV + SUSP_ADD):
        return "mid"
    return "light"


def light_min_n(k):
    """fewest kept rows at which a column with largest alt count k is still light (k < MID_K)"""
    if k < SUSP_FLOOR:
        return k
    return (k - SUSP_ADD + 1) * SUSP_DIV


def seg_class(k):
    return next((i for i, b in enumerate(SEG_CLASS_MAXK) if k <= b), len(SEG_CLASS_MAXK))


def lut_p(q):
    """the double the quality LUT holds for Phred q (fill_luts: pow(10.0, -1.0 * q / 10.0))"""
    return 10.0 ** (-1.0 * q / 10.0)


# ---- the column builder ---------------------------------------------------------------------------------------------

def edge_column(n, counts, q=30, ref=b"A", alt_at="first", q2=None, n_q2=0, low_bq_every=0, low_bq=2, low_bq_tail=0):
    """A column with n kept rows, filtered alt counts `counts` = (k0, k1, k2) (alleles in ACGT order after the reference),
    every kept row at quality q except n_q2 reference rows at q2; BAQ missing, MQ NA, so every merged error probability
    is lut_p(q) (or lut_p(q2)).
      alt_at:        "first" / "last": the alt rows lead / close the column; "spread": evenly through it
      low_bq_every:  after every that many kept rows a row of quality low_bq < MIN_BQ (a reference base) that the filter
                     drops -- raw row indices run ahead of the kept ones; low_bq_tail more such rows close the column"""
    counts = tuple(int(x) for x in counts)
    n_alt = sum(counts)
    assert n_alt <= n and n_q2 <= n - n_alt and low_bq < MIN_BQ
    ref_code = b"ACGT".index(ref)
    alts = [x for x in range(4) if x != ref_code]
    alt_codes = np.concatenate([np.full(c, alts[a], np.int64) for a, c in enumerate(counts)])
    if alt_at == "first":
        pos = np.arange(n_alt)
    elif alt_at == "last":
        pos = np.arange(n - n_alt, n)
    elif alt_at == "spread":
        pos = (np.arange(n_alt) * n) // max(n_alt, 1)
    else:
        raise ValueError(alt_at)
    code = np.full(n, ref_code, np.int64)
    code[pos] = alt_codes
    bq = np.full(n, q, np.uint8)
    if n_q2:
        ref_rows = np.nonzero(code == ref_code)[0]
        bq[ref_rows[(np.arange(n_q2) * len(ref_rows)) // n_q2]] = q2
    if low_bq_every:
        n_low = (n - 1) // low_bq_every
        at = (np.arange(n_low) + 1) * low_bq_every           # insert before kept row `at`
        code = np.insert(code, at, ref_code)
        bq = np.insert(bq, at, low_bq)
    if low_bq_tail:
        code = np.concatenate([code, np.full(low_bq_tail, ref_code, np.int64)])
        bq = np.concatenate([bq, np.full(low_bq_tail, low_bq, np.uint8)])
    nt = code.astype(np.uint8)
    nt[1::2] |= 8
    m = len(nt)
    return dict(nt=nt, bq=bq.astype(np.uint8), baq=np.full(m, 255, np.uint8), mq=np.full(m, 255, np.uint8), sq=None,
                col_off=np.array([0, m], np.uint64), ref_base=np.frombuffer(ref, np.uint8).copy(),
                spec=dict(n=n, counts=counts, q=q, q2=q2, n_q2=n_q2))


def batch_of(cols):
    host = util.concat_batches(cols)
    host["specs"] = [c["spec"] for c in cols]
    return host


# ---- the exact tail -------------------------------------------------------------------------------------------------

DPS = 60


def _binom_tail(k, n, p):
    """P(Bin(n, p) >= k) as an mpf, summed term by term (either tail, whichever is the short sum of positive terms)"""
    if k <= 0:
        return mpmath.mpf(1)
    if k > n:
        return mpmath.mpf(0)
    p = mpmath.mpf(p)
    q = 1 - p
    eps = mpmath.mpf(10) ** (-DPS - 5)
    mean = float(n * p)
    if k - 1 >= mean:                   # upper tail: terms fall from k on
        t = mpmath.binomial(n, k) * p ** k * q ** (n - k)
        s, j, r = t, k, p / q
        while j < n:
            t = t * (n - j) / (j + 1) * r
            j += 1
            s += t
            if t < s * eps:
                break
        return s
    # below the mean: 1 - P(X <= k - 1), terms fall from k - 1 down
    j = k - 1
    t = mpmath.binomial(n, j) * p ** j * q ** (n - j)
    s, r = t, q / p
    while j > 0:
        t = t * j / (n - j + 1) * r
        j -= 1
        s += t
        if t < s * eps:
            break
    return 1 - s


def exact_tail(k, spec):
    """P(X >= k) for a column of edge_column(**spec): X = Bin(n - n_q2, lut_p(q)) + Bin(n_q2, lut_p(q2)).
    A spec may give the probability of the body as "p" instead of "q" (a merged probability is no LUT value), and rows at
    further levels as "levels": [(rows, probability)] -- X is then the sum of all those binomials."""
    with mpmath.workdps(DPS):
        n = spec["n"]
        p1 = spec["p"] if "p" in spec else lut_p(spec["q"])
        levels = [(int(r), mpmath.mpf(p)) for r, p in spec.get("levels", ())]
        if spec.get("n_q2", 0):
            levels.append((spec["n_q2"], mpmath.mpf(lut_p(spec["q2"]))))
        if not levels:
            return _binom_tail(k, n, p1)
        pmf = [mpmath.mpf(1)]                           # of the rows beside the body
        for rows, p in levels:
            b = [mpmath.binomial(rows, j) * p ** j * (1 - p) ** (rows - j) for j in range(rows + 1)]
            pmf = [mpmath.fsum(pmf[i] * b[j - i] for i in range(max(0, j - rows), min(j, len(pmf) - 1) + 1))
                   for j in range(len(pmf) + rows)]
        body = n - sum(r for r, _ in levels)
        return mpmath.fsum(w * _binom_tail(k - j, body, p1) for j, w in enumerate(pmf))


def exact_log_tail(k, spec):
    with mpmath.workdps(DPS):
        return float(mpmath.log(exact_tail(k, spec)))


def log_close(logp_dev, logp_exact, n_obs):
    """the bar of util.assert_pvalue_close for a p-value whose exact log is logp_exact"""
    return util.PV_LOG_TOL if abs(logp_exact) <= util.PV_DEEP_LOG else util.pv_deep_bound(logp_exact, n_obs)


def n_for_tail(k, q, target, lo=None, hi=200000):
    """smallest kept-row count n >= lo at which P(Bin(n, lut_p(q)) >= k) >= target (the tail grows with n)"""
    lo = max(k, lo or k)
    with mpmath.workdps(30):
        assert _binom_tail(k, hi, lut_p(q)) >= target
        while lo < hi:
            mid = (lo + hi) // 2
            if _binom_tail(k, mid, lut_p(q)) >= target:
                hi = mid
            else:
                lo = mid + 1
    return lo


# ---- the boundary table ---------------------------------------------------------------------------------------------

Edge = namedtuple("Edge", "boundary const at n k q cls route opts")


def _mid_plan_chunks():
    """m such that a mid column of 64 m rows has m chunks and one of 64 m + 1 rows has m + 1, where lfq_split_plan's
    answer changes after the LFQ_PHASE1_CHUNKS stretch: rows after the stretch at all (rem = 0 -> 1), the first split
    (rem = 2 * LFQ_SEG_MIN_CHUNKS_SHORT) and the long minimum taking over (rem = LFQ_SEG_SHORT_BELOW)"""
    short = C["LFQ_SEG_MIN_CHUNKS_SHORT"][0]
    below = C["LFQ_SEG_SHORT_BELOW"][0]
    return [PHASE1, PHASE1 + 2 * short - 1, PHASE1 + below - 1]


def _big_plan_chunks():
    """the same for a big column (no phase-1 stretch): the first split, the long minimum"""
    short = C["LFQ_SEG_MIN_CHUNKS_SHORT"][0]
    below = C["LFQ_SEG_SHORT_BELOW"][0]
    return [2 * short - 1, below - 1]


def kept_for_raw(raw, every):
    """(n, tail): edge_column(n, ..., low_bq_every=every, low_bq_tail=tail) has `raw` rows in all"""
    n = raw
    while n + (n - 1) // every > raw:
        n -= 1
    return n, raw - (n + (n - 1) // every)


def boundary_table():
    """every boundary of the routing rule as a list of Edge: a column of n kept rows whose largest filtered alt count is k,
    every kept row at quality q, which must take class `cls`; `route` names the kernel path; `opts` are edge_column options"""
    t = []

    def add(boundary, const, n, k, q, cls=None, route=None, **opts):
        c = dp_class(k, n)
        assert cls is None or c == cls, (boundary, n, k, c, cls)
        if route is None:
            route = {"light": "light-screen" if k <= SCREEN_MAXK[-1] else "light-wave", "mid": "mid",
                     "big": "big-split" if k <= SPLIT_MAX_K else "big-unsplit"}[c]
        t.append(Edge(boundary, const, C[const][1], n, k, q, c, route, opts))

    # light / mid at LFQ_MID_K and the suspicious rule max(FLOOR, n / DIV + ADD)
    k = MID_K - 1
    n = light_min_n(k)
    add("light/mid: suspicious at K = MID_K - 1", "suspicious", n, k, 30, "light")
    add("light/mid: suspicious at K = MID_K - 1", "suspicious", n - 1, k, 30, "mid")
    add("light/mid: K = MID_K", "LFQ_MID_K", n + 1, MID_K, 30, "mid")
    add("light/mid: suspicious floor", "suspicious", 200, SUSP_FLOOR - 1, 20, "light")
    add("light/mid: suspicious floor", "suspicious", 200, SUSP_FLOOR, 20, "mid")
    n = light_min_n(SUSP_FLOOR + 1)
    add("light/mid: suspicious above the floor", "suspicious", n, SUSP_FLOOR + 1, 20, "light", alt_at="last")
    add("light/mid: suspicious above the floor", "suspicious", n - 1, SUSP_FLOOR + 1, 20, "mid", alt_at="last")
    # mid / big at LFQ_BIG_K
    add("mid/big: K = BIG_K - 1", "LFQ_BIG_K", 2000, BIG_K - 1, 10, "mid")
    add("mid/big: K = BIG_K", "LFQ_BIG_K", 2000, BIG_K, 10, "big")
    # the screen variants: MAXK - 1, MAXK, MAXK + 1 of every one, light
    for maxk in SCREEN_MAXK:
        n = max(light_min_n(maxk + 1), 4 * maxk)
        for kk in (maxk - 1, maxk, maxk + 1):
            add("screen KREG = %d: K = MAXK%+d" % (maxk + 1, kk - maxk), "lfq_khist_thr", n, kk, 6, "light", alt_at="spread")
    # cells-per-lane classes of a row segment, each side of every class bound (mid: split after the phase-1 stretch)
    for b in SEG_CLASS_MAXK:
        for kk in (b, b + 1):
            n = max(4 * kk, 64 * (PHASE1 + 40))
            add("segment class: K = %d" % kk, "lfq_seg_class", n, kk, 6, "mid" if kk < BIG_K else "big")
    # nothing is split above LFQ_SPLIT_MAX_K
    add("split: K = SPLIT_MAX_K", "LFQ_SPLIT_MAX_K", 8100, SPLIT_MAX_K, 6, "big", route="big-split")
    add("split: K = SPLIT_MAX_K + 1", "LFQ_SPLIT_MAX_K", 8100, SPLIT_MAX_K + 1, 6, "big", route="big-unsplit")
    # fold: the narrow convolution up to K = 128; the combine kernel's slow path above its KMAX (252 / 1008)
    fk = C["fold K"][0]
    for kk in (fk, fk + 1):
        add("fold: K = %d" % kk, "fold K", 3000, kk, 6, "mid")
    for km in C["combine KMAX"][0]:
        for kk in (km, km + 1):
            add("combine: K = %d" % kk, "combine KMAX", max(4 * kk, 4000), kk, 6)
    # the unsplit big kernel: 2 cells per lane below 128 * NW - 1, 4 above; 4 cells fill the NW strips of one pass up
    # to K = 4 * (64 * NW) - 4, a second pass above
    c2 = C["big C=2 below"][0]
    for kk in (c2 - 1, c2):
        add("big kernel: K = %d (C = %d)" % (kk, 2 if kk < c2 else 4), "big C=2 below", 4 * kk, kk, 6)
    one_pass = 4 * 64 * C["LFQ_HEAVY_WAVES"][0] - 4
    for kk in (one_pass, one_pass + 1):
        add("big kernel: K = %d, %d pass(es)" % (kk, 1 if kk == one_pass else 2), "LFQ_HEAVY_WAVES", 4 * kk, kk, 6,
            "big", route="big-unsplit")
    # split plan: N = 64 m - 1, 64 m, 64 m + 1 at the chunk counts where the plan changes; once with raw rows, once with
    # rows below min_bq interleaved (raw index > kept index)
    for m in _mid_plan_chunks():
        for n in (64 * m - 1, 64 * m, 64 * m + 1):
            add("split plan (mid): %d chunks %+d" % (m, n - 64 * m), "LFQ_PHASE1_CHUNKS" if m == PHASE1 else "LFQ_SEG_MIN_CHUNKS_SHORT" if m < PHASE1 + C["LFQ_SEG_SHORT_BELOW"][0] - 1 else "LFQ_SEG_SHORT_BELOW",
                n, 100, 6, "mid", alt_at="last")
    for m in _big_plan_chunks():
        for n in (64 * m - 1, 64 * m, 64 * m + 1):
            add("split plan (big): %d chunks %+d" % (m, n - 64 * m), "LFQ_SEG_MIN_CHUNKS_SHORT" if m < C["LFQ_SEG_SHORT_BELOW"][0] - 1 else "LFQ_SEG_SHORT_BELOW",
                n, BIG_K, 6, "big", alt_at="last")
    m = _mid_plan_chunks()[1]
    for raw in (64 * m - 1, 64 * m, 64 * m + 1):
        n, tail = kept_for_raw(raw, 7)
        add("split plan (mid), low-BQ rows interleaved: raw rows %d chunks %+d (%d kept)" % (m, raw - 64 * m, n),
            "LFQ_SEG_MIN_CHUNKS_SHORT", n, 100, 6, "mid", alt_at="spread", low_bq_every=7, low_bq_tail=tail)
    for n in (64 * m - 1, 64 * m, 64 * m + 1):
        add("split plan (mid), low-BQ rows interleaved: kept rows %d chunks %+d" % (m, n - 64 * m), "LFQ_SEG_MIN_CHUNKS_SHORT",
            n, 100, 6, "mid", alt_at="last", low_bq_every=5)
    return t


def table_column(e, shape=None):
    """the table row as a column; shape: the (k0, k1, k2) counts (default (K, 0, 0)); max(shape) must be K"""
    counts = shape or (e.k, 0, 0)
    assert max(counts) == e.k
    return edge_column(e.n, counts, q=e.q, **e.opts)


def multi_shapes(k):
    """multi-allele shapes with largest count k"""
    return [(k, k, 1), (k, k - 1, 0), (1, 0, k)] if k >= 2 else [(0, 1, 0)]


# ---- knife edges: columns whose exact p * bonferroni falls just either side of sig ------------------------------------

# (route, K, q, fewest kept rows, conf) of one knife-edge family per route
KNIFE_ROUTES = [
    ("light-screen LB", 5, 30, 0, {}),
    ("light-screen exact", 5, 30, 0, dict(def_alt_bq=-1)),
    ("light-wave", 40, 33, light_min_n(40), {}),
    ("mid", 100, 20, 0, {}),
    ("big-split", 300, 15, 0, {}),
    ("big-unsplit", SPLIT_MAX_K + 84, 10, 0, {}),
]
KNIFE_SLACK = 5e-7          # inside prune_slack (1e-6): the device keeps the column, the host's exact test decides
KNIFE_MARGIN = 1e-5         # a pair's columns at least this far (relative) from sig / bonf


def _bonf_between(p_lo, p_hi):
    b = int(round(SIG / float(mpmath.sqrt(p_lo * p_hi))))
    assert p_lo * b < SIG * (1 - KNIFE_MARGIN) and p_hi * b > SIG * (1 + KNIFE_MARGIN), (p_lo, p_hi, b)
    return b


def knife_batches():
    """per route: [dict(route, name, cols, bonf, emit, conf)] -- `emit[i]`: column i must be called (its exact
    p * bonf < sig); bonf_dynamic = 0, bonf_subst = bonf"""
    out = []
    with mpmath.workdps(DPS):
        for route, k, q, n_min, conf in KNIFE_ROUTES:
            alt_at = "spread" if "light" in route else "last"
            n = n_for_tail(k, q, 1e-7, lo=n_min)
            a, b = edge_column(n, (k, 0, 0), q=q, alt_at=alt_at), edge_column(n + 1, (k, 0, 0), q=q, alt_at=alt_at)
            pa, pb = exact_tail(k, a["spec"]), exact_tail(k, b["spec"])
            out.append(dict(route=route, name="N / N + 1", cols=[a, b], bonf=_bonf_between(pa, pb), emit=[True, False]))
            c = edge_column(n, (k, 1, 0), q=q, alt_at=alt_at, q2=q - 3, n_q2=3, low_bq_every=11)
            pc = exact_tail(k, c["spec"])
            out.append(dict(route=route, name="second quality level", cols=[c, a], bonf=_bonf_between(pa, pc),
                            emit=[False, True]))
            n = n_for_tail(k, q, 1e-11, lo=n_min)
            s = edge_column(n, (k, 0, 0), q=q, alt_at=alt_at)
            ps = exact_tail(k, s["spec"])
            for side in (-1, 1):
                bonf = int(round(SIG * (1 + side * KNIFE_SLACK) / ps))
                r = float(ps * bonf / SIG - 1)
                assert abs(r - side * KNIFE_SLACK) < 2e-9 and bonf > 10 ** 8, (route, r, bonf)
                out.append(dict(route=route, name="p * B / sig = 1 %+.0e" % (side * KNIFE_SLACK), cols=[s], bonf=bonf,
                                emit=[side < 0]))
        for kb in out:
            kb["conf"] = dict(next(r[4] for r in KNIFE_ROUTES if r[0] == kb["route"]), bonf_dynamic=0, bonf_subst=kb["bonf"])
    return out
