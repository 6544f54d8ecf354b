"""Batches at the routing and chunk boundaries of the count -> scan stage (lfq_kernels.hip: lfq_launch_count and the kernels
it chooses among, lfq_maxdepth_kernel, lfq_scan_*).

Used by test_count_edges.py (CPU: the restatement against the oracle, the builder, the routing rule) and
test_gpu_count_edges.py (every row on the kernel it must take):

  source_constants  the routing constants and the kernels' geometry, read from the sources with file:line;
  expected_kernel   lfq_launch_count / lfq_count_is_shallow / lfq_count_is_lean restated: the instantiation a batch takes;
  counts_ref        plp_to_errprobs' integer outputs (snpcaller.c:346-498) and the gates of call_snvs / call_vars
                    (lofreq_call.c:747-801) for the default filters, in plain numpy;
  edge_batch        host tracks with exact column lengths, start residues mod 16, reference bases, alt positions and
                    qualities;
  boundary_table    name -> batch, configuration, the kernel each route must take, and why the row is there.
"""
import os
import re
from collections import namedtuple

import numpy as np

import dp_edges as de

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")

MIN_BQ, MIN_ALT_BQ, MIN_COV = 6, 6, 1       # lfq_conf_init
ROUTES = ("dense/byte", "dense/packed", "lazy/byte", "lazy/packed")


# ---- the constants, read from the sources ----------------------------------------------------------------------------

def _find(fname, pattern):
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
    """{name: (value, 'file:line')}; a constant that is not found is an AssertionError"""
    c = {}
    for name, knob in (("count_lpg4_below", "LFQ_COUNT_LPG4_BELOW"), ("count_lpg8_below", "LFQ_COUNT_LPG8_BELOW"),
                       ("count_multi_below", "LFQ_COUNT_MULTI_BELOW")):
        m, at = _find("lfq_host.cpp", r"x\.%s = LFQ_TUNE_I\(\"%s\", (\d+)\);" % (name, knob))
        c[name] = (int(m.group(1)), at)
    for name in ("LFQ_COUNT_AHEAD", "LFQ_COUNT_WG_WAVES", "LFQ_SCAN_THREADS", "LFQ_SCAN_ITEMS", "LFQ_NLO_PACK"):
        c[name] = _define("lfq_kernels.hip", name)
    for name in ("LFQ_BOUND_QLO", "LFQ_BOUND_SUBSET", "LFQ_BOUND_SHIFT"):
        c[name] = _define("lfq_bound.h", name)
    # lfq_launch_maxdepth: min((ncols + 255) / 256, 1024) workgroups of 256 lanes
    m, at = _find("lfq_kernels.hip", r"std::min<int64_t>\(\(t\.ncols \+ 255\) / (\d+), (\d+)\);")
    c["maxdepth grid"] = ((int(m.group(2)), int(m.group(1))), at)
    # the shallow kernel: 256 columns per workgroup and pass, at most 256 * 8 * 4 workgroups
    m, at = _find("lfq_kernels.hip", r"blocks64 = \(c1 - c0 \+ 255\) / (\d+);")
    c["shallow columns per workgroup"] = (int(m.group(1)), at)
    m, at = _find("lfq_kernels.hip", r"std::min<int64_t>\(blocks64, \(int64_t\)(\d+) \* (\d+) \* (\d+)\);")
    c["shallow workgroup cap"] = (int(m.group(1)) * int(m.group(2)) * int(m.group(3)), at)
    # rounds = (max_col_obs / 16 + 2 + AHEAD * lpg - 1) / (AHEAD * lpg)
    m, at = _find("lfq_kernels.hip", r"rounds = \(int\)\(\(max_col_obs / 16 \+ (\d+) \+ LFQ_COUNT_AHEAD \* lpg - 1\) / "
                                     r"\(LFQ_COUNT_AHEAD \* lpg\)\);")
    c["rounds slack"] = (int(m.group(1)), at)
    m, at = _find("lfq_kernels.hip", r"const int lpg = max_col_obs <= kn\.count_lpg4_below \? (\d+) : "
                                     r"max_col_obs <= kn\.count_lpg8_below \? (\d+) : (\d+);")
    c["lanes per column"] = (tuple(int(x) for x in m.groups()), at)
    # the lean kernel's loop: chunks in flight per lane
    m, at = _find("lfq_kernels.hip", r"constexpr int UNROLL = (\d+); +/\* chunks in flight per lane, as in lfq_count_column_fast")
    c["lean UNROLL"] = (int(m.group(1)), at)
    return c


C = source_constants()
LPG4_BELOW, LPG8_BELOW, MULTI_BELOW = (C[k][0] for k in ("count_lpg4_below", "count_lpg8_below", "count_multi_below"))
AHEAD = C["LFQ_COUNT_AHEAD"][0]
LPGS = C["lanes per column"][0]
SCAN_TILE = C["LFQ_SCAN_THREADS"][0] * C["LFQ_SCAN_ITEMS"][0]
WG_WAVES = C["LFQ_COUNT_WG_WAVES"][0]
Q_LO = C["LFQ_BOUND_QLO"][0]               # the bound gate's statistic counts kept rows of bq <= 31
# the deepest column a batch of each lanes-per-column setting can have
LPG_MAX_DEPTH = dict(zip(LPGS, (LPG4_BELOW, LPG8_BELOW, MULTI_BELOW - 1)))


# ---- the routing rule -----------------------------------------------------------------------------------------------

def expected_kernel(max_col_obs, packed, dense_strand, same_thr, general=False, detlim=False):
    """the instantiation lfq_launch_count launches for a batch whose deepest column has max_col_obs observations.
    packed: the nt layout; dense_strand: strand counts asked of every column (LfqParams::lazy_strand off); same_thr:
    min_alt_bq == min_bq; general: merged-quality filters or the median override; detlim: lofreq uniq's detection limit"""
    b = lambda x: "true" if x else "false"
    default = not general and not detlim
    lazy = default and not dense_strand                     # lfq_batch_device_impl: P.lazy_strand
    if default and 0 < max_col_obs < MULTI_BELOW:
        lpg = LPGS[0] if max_col_obs <= LPG4_BELOW else LPGS[1] if max_col_obs <= LPG8_BELOW else LPGS[2]
        if packed:                                          # lfq_count_is_shallow
            return "lfq_count_shallow_kernel<%s, %d>" % (b(not lazy), lpg)
        return "lfq_count_multi_kernel<false, %s, %d>" % (b(not lazy), lpg)
    strand = not lazy or general
    if default:
        if packed and lazy:                                 # lfq_count_is_lean
            return "lfq_count_lean_kernel<%s>" % b(same_thr)
        return "lfq_count_fast_kernel<%s, %s, %s>" % (b(packed), b(strand), b(same_thr))
    return "lfq_count_kernel<%s, %s>" % (b(packed), b(strand))


def shallow_rounds(max_col_obs, lpg):
    return (max_col_obs // 16 + C["rounds slack"][0] + AHEAD * lpg - 1) // (AHEAD * lpg)


# ---- plp_to_errprobs' integer outputs, default filters ------------------------------------------------------------------

REF_FIELDS = ("n_err_probs", "alt_counts", "alt_raw_counts", "alt_fw", "ref_fw", "ref_rv", "kmax", "tested", "gated",
              "coverage")
LAZY_FIELDS = ("n_err_probs", "alt_counts", "kmax", "tested", "gated", "coverage")
REF_DTYPE = np.dtype([("n_err_probs", "i4"), ("alt_counts", "i4", 3), ("alt_raw_counts", "i4", 3), ("alt_fw", "i4", 3),
                      ("ref_fw", "i4"), ("ref_rv", "i4"), ("kmax", "i4"), ("tested", "u1"), ("gated", "u1"),
                      ("coverage", "i4")])


def counts_ref(host, conf=None):
    """REF_FIELDS of lfq_col_counts for every column of `host`, default filters only: conf may set min_bq, min_alt_bq and
    min_cov.  Per observation (snpcaller.c:383-498 with no merged-quality filter): codes above 3 are N and skipped; an alt
    base counts raw whatever its quality (:418-420); a base below min_bq is dropped (:426), an alt base below min_alt_bq
    too (:431-433); what is left is an error probability, and an alt one a filtered alt count.  Per column
    (lofreq_call.c:747-801, :892, :930): a reference base outside ACGT, 2 * num_bases < coverage_plp and
    num_bases < min_cov gate it; it is tested when a filtered alt count is non-zero."""
    conf = conf or {}
    assert not set(conf) - {"min_bq", "min_alt_bq", "min_cov"}, "counts_ref covers the default filters only"
    min_bq, min_alt_bq = conf.get("min_bq", MIN_BQ), conf.get("min_alt_bq", MIN_ALT_BQ)
    min_cov = conf.get("min_cov", MIN_COV)
    off = np.asarray(host["col_off"]).astype(np.int64)
    ncols = len(off) - 1
    lens = np.diff(off)
    n = int(off[-1])
    nt, bq = np.asarray(host["nt"][:n]), np.asarray(host["bq"][:n])
    rb = np.asarray(host["ref_base"][:ncols])
    ref_code = np.full(ncols, -1, np.int64)
    for x, ch in enumerate(b"ACGT"):
        ref_code[rb == ch] = x
    cov = lens if host.get("coverage_plp") is None else np.asarray(host["coverage_plp"]).astype(np.int64)
    nb = lens if host.get("num_bases") is None else np.asarray(host["num_bases"]).astype(np.int64)
    gated = (ref_code < 0) | (2 * nb < cov) | (nb < min_cov)

    code = (nt & 7).astype(np.int64)
    key = np.repeat(np.arange(ncols, dtype=np.int64), lens) * 4 + np.minimum(code, 3)
    valid = code <= 3
    fwd = (nt & 8) == 0
    per = lambda mask: np.bincount(key[mask], minlength=4 * ncols).reshape(ncols, 4)
    raw, fw = per(valid), per(valid & fwd)
    ge = per(valid & (bq >= min_bq))
    ga = per(valid & (bq >= min_bq) & (bq >= min_alt_bq))

    rc = np.maximum(ref_code, 0)
    cols = np.arange(ncols)
    alt_x = np.stack([np.where(rc == 0, 1, 0), np.where(rc <= 1, 2, 1), np.where(rc <= 2, 3, 2)], axis=1)   # snpcaller.c:391-397
    out = np.zeros(ncols, REF_DTYPE)
    live = ~gated
    out["alt_counts"] = np.take_along_axis(ga, alt_x, 1) * live[:, None]
    out["alt_raw_counts"] = np.take_along_axis(raw, alt_x, 1) * live[:, None]
    out["alt_fw"] = np.take_along_axis(fw, alt_x, 1) * live[:, None]
    out["ref_fw"] = fw[cols, rc] * live
    out["ref_rv"] = (raw[cols, rc] - fw[cols, rc]) * live
    out["n_err_probs"] = (ge[cols, rc] + out["alt_counts"].sum(1)) * live
    out["kmax"] = out["alt_counts"].max(1)
    out["tested"] = out["kmax"] > 0
    out["gated"] = gated
    out["coverage"] = cov
    return out


# ---- the batch builder ----------------------------------------------------------------------------------------------

def col(n, res=None, ref="A", alts="none", q="mix", low=(), n_every=11, cov=None, nb=None, tag=""):
    """one column of an edge_batch:
      n        observations
      res      the residue mod 16 its first observation must have (None: wherever it falls)
      ref      the reference base, any character ('N', a lower-case letter)
      alts     "none"; "ends": the first and the last observation; "edges": those and both sides of every boundary
               between two 16-observation chunks of the tracks; or a list of positions
      q        "mix": qualities either side of min_bq, min_alt_bq and the bound gate's 31 / 32, and 93, drawn at random,
               the alt bases' cycling through the same; a number: that quality everywhere
      low      positions (reference bases) set to quality 20
      n_every  every that many-th observation that is no alt base gets one of the codes 4..7 (0: none)
      cov, nb  coverage_plp / num_bases of the column (edge_batch(..., with_cov=True); None: n + 1 / n)"""
    return dict(n=int(n), res=res, ref=ref, alts=alts, q=q, low=tuple(int(x) for x in low), n_every=n_every, cov=cov, nb=nb,
                tag=tag)


def edge_batch(cols, seed=1, min_bq=MIN_BQ, min_alt_bq=MIN_ALT_BQ, with_cov=False):
    """host tracks of the columns `cols` (col(...)), with a filler column of 1..15 reference observations in front of a
    column whose start would not have the residue it asks for.  host["index"][i]: the column of cols[i]; host["specs"][c]:
    what column c was built from, with its start, its alt positions and their codes (fillers: tag "filler")."""
    rng = np.random.default_rng(seed)
    palette = np.array([min_bq - 1, min_bq, min_alt_bq - 1, min_alt_bq, Q_LO, Q_LO + 1, 93, 20, 40, 40, 40, 40], np.uint8)
    alt_q = np.array([min_alt_bq, Q_LO, Q_LO + 1, 93, 40, min_alt_bq - 1, min_bq - 1, 40], np.uint8)
    nts, bqs, lens, refs, specs, index, covs, nbs = [], [], [], [], [], [], [], []
    start = 0

    def put(c, nt, bq, spec):
        nonlocal start
        nts.append(nt)
        bqs.append(bq)
        lens.append(len(nt))
        refs.append(ord(c["ref"]))
        covs.append(len(nt) + 1 if c["cov"] is None else c["cov"])
        nbs.append(len(nt) if c["nb"] is None else c["nb"])
        specs.append(dict(spec, start=start, n=len(nt), ref=c["ref"], tag=c["tag"], res=c["res"]))
        start += len(nt)

    for c in cols:
        if c["res"] is not None and start % 16 != c["res"]:
            m = (c["res"] - start) % 16
            f = col(m, tag="filler")
            put(f, (np.arange(m) % 2 * 8).astype(np.uint8), np.full(m, 40, np.uint8), dict(alt_pos=(), alt_code=()))
        n = c["n"]
        ref_code = "ACGT".find(c["ref"])
        base = max(ref_code, 0)
        if isinstance(c["alts"], str):
            pos = set()
            if c["alts"] in ("ends", "edges") and n:
                pos |= {0, n - 1}
            if c["alts"] == "edges":
                p = np.arange(n)
                pos |= set(p[np.isin((start + p) % 16, (15, 0))].tolist())
        else:
            pos = set(int(x) for x in c["alts"])
        pos = np.array(sorted(pos), np.int64)
        assert pos.size == 0 or (0 <= pos.min() and pos.max() < n)
        code = np.full(n, base, np.uint8)
        others = np.array([x for x in range(4) if x != base], np.uint8)
        acode = others[np.arange(pos.size) % 3]
        code[pos] = acode
        if c["q"] == "mix":
            bq = palette[rng.integers(0, len(palette), n)]
            bq[pos] = alt_q[np.arange(pos.size) % len(alt_q)]
        else:
            bq = np.full(n, c["q"], np.uint8)
        if c["low"]:
            low = np.array(c["low"], np.int64)
            assert not np.isin(low, pos).any()
            bq[low] = 20
        if c["n_every"]:
            isn = np.arange(n) % c["n_every"] == c["n_every"] - 1
            isn[pos] = False
            code[isn] = (4 + np.arange(n) % 4)[isn]
        nt = code | (rng.integers(0, 2, n).astype(np.uint8) << 3)
        index.append(len(lens))
        put(c, nt, bq, dict(alt_pos=tuple(pos.tolist()), alt_code=tuple(acode.tolist())))
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.uint8)
    total = int(np.sum(lens))
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    host = dict(nt=cat(nts), bq=cat(bqs), baq=np.full(total, 255, np.uint8), mq=np.full(total, 255, np.uint8), sq=None,
                col_off=off, ref_base=np.array(refs, np.uint8), specs=specs, index=np.array(index, np.int64))
    if with_cov:
        host["coverage_plp"] = np.array(covs, np.int32)
        host["num_bases"] = np.array(nbs, np.int32)
    return host


def class_column(cls, ref=b"A"):
    """the smallest column of a DP class that is called at any Bonferroni factor a test here reaches (dp_edges.dp_class)"""
    k = {"light": 3, "mid": de.SUSP_FLOOR, "big": de.BIG_K}[cls]
    n = k + 50
    assert de.dp_class(k, n) == cls
    return de.edge_column(n, (k, 0, 0), q=30, ref=ref, alt_at="first")


# ---- the table ----------------------------------------------------------------------------------------------------------

# name; group; the source constants its geometry comes from; build() -> host; conf overrides; {route: kernel it must take};
# why it is there; extra checks for the GPU test
Row = namedtuple("Row", "name group consts build conf kernels why checks")

_SHORT = (0, 1, 2, 3, 5, 8, 13, 15, 16, 17, 21, 31, 32, 33, 40, 47, 64, 7)
_REFS = "ACGTACGNTgCA"
_ALTS = ("ends", "none", "edges", "ends", "none")


def _short_cols(k, shift=0, res=None):
    return [col(_SHORT[(i + shift) % len(_SHORT)], res=res, ref=_REFS[(i + shift) % len(_REFS)],
                alts=_ALTS[(i + shift) % len(_ALTS)]) for i in range(k)]


def _deep(n, res=15, ref="C"):
    """the column that decides the batch's route: its last observation an alt base, its start at residue 15"""
    return col(n, res=res, ref=ref, alts="edges", tag="deep")


def _kernels(max_col_obs, same_thr, general=False, routes=ROUTES):
    return {r: expected_kernel(max_col_obs, r.endswith("packed"), r.startswith("dense"), same_thr, general) for r in routes}


def _routing_rows(t):
    b = lambda x: "true" if x else "false"
    claims = {
        # the deepest column: (the constant it sits next to, lanes per column; None: not a shared-wavefront kernel)
        LPG4_BELOW: ("count_lpg4_below", 4), LPG4_BELOW + 1: ("count_lpg4_below", 8),
        LPG8_BELOW: ("count_lpg8_below", 8), LPG8_BELOW + 1: ("count_lpg8_below", 16),
        MULTI_BELOW - 1: ("count_multi_below", 16), MULTI_BELOW: ("count_multi_below", None),
    }
    for n, (const, lpg) in claims.items():
        for same_thr in (True, False):
            conf = {} if same_thr else dict(min_bq=6, min_alt_bq=10)
            if lpg:
                k = {"dense/byte": "lfq_count_multi_kernel<false, true, %d>" % lpg,
                     "dense/packed": "lfq_count_shallow_kernel<true, %d>" % lpg,
                     "lazy/byte": "lfq_count_multi_kernel<false, false, %d>" % lpg,
                     "lazy/packed": "lfq_count_shallow_kernel<false, %d>" % lpg}
            else:
                k = {"dense/byte": "lfq_count_fast_kernel<false, true, %s>" % b(same_thr),
                     "dense/packed": "lfq_count_fast_kernel<true, true, %s>" % b(same_thr),
                     "lazy/byte": "lfq_count_fast_kernel<false, false, %s>" % b(same_thr),
                     "lazy/packed": "lfq_count_lean_kernel<%s>" % b(same_thr)}
            checks = dict(routing=True, max_col_obs_0=True)
            if n in (MULTI_BELOW - 1, MULTI_BELOW):
                checks["sparse_entries"] = "kept" if n < MULTI_BELOW else "written"
            build = (lambda n=n, conf=conf: edge_batch(_short_cols(35) + [_deep(n)] + _short_cols(35, 7), seed=n,
                                                       min_bq=conf.get("min_bq", MIN_BQ), min_alt_bq=conf.get("min_alt_bq", MIN_ALT_BQ)))
            t.append(Row("routing/%d/%s" % (n, "one_thr" if same_thr else "two_thr"), "routing", (const,), build, conf, k,
                         "the deepest column has %d observations: %s = %d" % (n, const, C[const][0]), checks))
    # the general path: every observation evaluated, whatever the depth
    t.append(Row("routing/general/min_jq", "routing", ("count_multi_below",),
                 lambda: edge_batch(_short_cols(35) + [_deep(MULTI_BELOW)] + _short_cols(35, 7), seed=11), dict(min_jq=1),
                 {r: "lfq_count_kernel<%s, true>" % b(r.endswith("packed")) for r in ROUTES},
                 "min_jq > 0: merged-quality filter, lfq_count_kernel at a depth that would take the lean kernel",
                 dict(routing=True, general=True, max_col_obs_0=True)))
    t.append(Row("routing/general/def_alt_bq", "routing", ("count_lpg4_below",),
                 lambda: edge_batch(_short_cols(35) + [_deep(LPG4_BELOW + 1)] + _short_cols(35, 7), seed=12), dict(def_alt_bq=-1),
                 {r: "lfq_count_kernel<%s, true>" % b(r.endswith("packed")) for r in ROUTES},
                 "def_alt_bq = -1: the median override, lfq_count_kernel at a depth that would take the shallow kernel",
                 dict(routing=True, general=True, median=True, max_col_obs_0=True)))


def shallow_lengths(lpg):
    """column lengths for a batch of `lpg` lanes per column: the first chunks, and the last chunk of a round / the first of
    the next (a round: AHEAD chunks per lane), as far as the routing constants let a column of this batch reach"""
    out = [0, 1, 15, 16, 17, 31, 32, 33]
    for r in (1, 2):
        for d in (-17, -16, -15, -1, 0, 1):
            n = 16 * AHEAD * lpg * r + d
            if n <= LPG_MAX_DEPTH[lpg]:
                out.append(n)
    return out


def _shallow_rows(t):
    for lpg in LPGS:
        deep = LPG_MAX_DEPTH[lpg]
        const = {4: "count_lpg4_below", 8: "count_lpg8_below", 16: "count_multi_below"}[lpg]
        kern = _kernels(deep, True)
        assert kern["dense/packed"] == "lfq_count_shallow_kernel<true, %d>" % lpg
        consts = (const, "LFQ_COUNT_AHEAD", "rounds slack", "lanes per column")

        def lengths(lpg=lpg, deep=deep):
            cols = []
            for i, n in enumerate(shallow_lengths(lpg)):
                for res in (0, 1, 8, 15):
                    cols.append(col(n, res=res, ref="ACGT"[(i + res) % 4], alts="edges"))
            return edge_batch(cols[: len(cols) // 2] + [_deep(deep)] + cols[len(cols) // 2:], seed=100 + lpg)
        t.append(Row("shallow/lpg%d/lengths" % lpg, "shallow", consts, lengths, {}, kern,
                     "chunk and round boundaries at start residues 0, 1, 8, 15; the deepest column (%d, %d rounds) at residue 15, "
                     "its last observation an alt base" % (deep, shallow_rounds(deep, lpg)), {}))
        # the batch's deepest column one observation short of, and at, a whole number of rounds, at residue 15: it touches
        # two chunks more than max_col_obs / 16, which is what the slack in `rounds` pays for
        lo = {4: 0, 8: LPG4_BELOW, 16: LPG8_BELOW}[lpg]
        for r in (1, 2):
            for d in (-1, 0):
                n = 16 * AHEAD * lpg * r + d
                if not lo < n <= deep:
                    continue
                assert (15 + n + 15) // 16 == n // 16 + C["rounds slack"][0] - (d == 0) and shallow_rounds(n, lpg) == r + 1
                t.append(Row("shallow/lpg%d/deepest%d" % (lpg, n), "shallow", consts,
                             lambda n=n: edge_batch(_short_cols(20) + [_deep(n)] + _short_cols(20, 5), seed=n), {}, _kernels(n, True),
                             "the deepest column has %d observations, %d short of %d rounds, and starts at residue 15: %d chunks"
                             % (n, -d, r, (15 + n + 15) // 16), {}))
        g = 64 // lpg
        for tail in (1, 63, 64, 65):
            for kind in ("empty", "gated"):
                def placed(lpg=lpg, g=g, tail=tail, kind=kind):
                    rng = np.random.default_rng(tail)
                    cols = [col(int(rng.integers(17, 49)), ref="ACGT"[i % 4], alts="ends") for i in range(192 + tail)]
                    cols[70] = col({4: 300, 8: 800, 16: 2000}[lpg], ref="G", alts="edges", tag="deep")
                    special = [0, 64, 63, 127] + list(range(128 + g, 128 + 2 * g)) + list(range(192, 192 + tail))
                    for j, i in enumerate(special):
                        cols[i] = (col(0, tag="special") if kind == "empty" else
                                   col(20 + j % 9, ref="NtnR"[j % 4], alts="edges", tag="special"))
                    return edge_batch(cols, seed=200 + tail)
                t.append(Row("shallow/lpg%d/%s/tail%d" % (lpg, kind, tail), "shallow", consts, placed, {},
                             _kernels({4: 300, 8: 800, 16: 2000}[lpg], True),
                             "%s columns at lane 0 and the last lane of a pass, a whole group of %d, and the last %d of the batch"
                             % (kind, g, tail), {}))
        for ncols in (1, 63, 64, 65, 255, 256, 257):
            def sized(deep=deep, ncols=ncols):
                rng = np.random.default_rng(ncols)
                cols = [_deep(deep, res=None)] + [col(int(rng.integers(0, 61)), ref="ACGT"[i % 4], alts=_ALTS[i % 5])
                                                  for i in range(ncols - 1)]
                return edge_batch(cols, seed=300 + ncols)
            t.append(Row("shallow/lpg%d/ncols%d" % (lpg, ncols), "shallow", consts, sized, {}, kern,
                         "a pass and a workgroup that end with idle lanes; the deepest column the route allows", {}))

        def gates(lpg=lpg):
            rng = np.random.default_rng(lpg)
            cols = [col(int(rng.integers(1, 61)), ref="ACGT"[i % 4], alts="ends") for i in range(100)]
            cols[5] = col({4: 300, 8: 800, 16: 2000}[lpg], ref="G", alts="edges", tag="deep")
            cols[10] = col(20, alts="ends", cov=40, nb=19, tag="2nb<cov")
            cols[20] = col(20, alts="ends", cov=40, nb=20, tag="2nb=cov")
            cols[30] = col(20, alts="ends", cov=0, nb=0, tag="nb<min_cov")
            cols[40] = col(20, alts="ends", cov=2, nb=1, tag="nb=min_cov")
            cols[63] = col(20, alts="ends", cov=41, nb=20, tag="2nb<cov")
            return edge_batch(cols, seed=400 + lpg, with_cov=True)
        t.append(Row("shallow/lpg%d/coverage_gates" % lpg, "shallow", consts, gates, {},
                     _kernels({4: 300, 8: 800, 16: 2000}[lpg], True),
                     "coverage_plp / num_bases given: 2 * nb < cov and nb < min_cov on single columns, both sides", dict(with_cov=True)))


LEAN_CHUNKS = (1, 2, 3, 65, 66, 67, 129, 130, 131, 257, 258, 259)


def lean_length(n_ch, res, last):
    """observations of a column that starts at residue `res`, touches n_ch chunks and has `last` observations in the last"""
    if n_ch == 1:
        return max(last - res, 1)
    return 16 * (n_ch - 1) - res + last


def _lean_rows(t):
    deep = MULTI_BELOW + 4
    consts = ("count_multi_below", "LFQ_COUNT_WG_WAVES", "lean UNROLL", "LFQ_NLO_PACK")
    for same_thr in (True, False):
        conf = {} if same_thr else dict(min_bq=6, min_alt_bq=10)

        def chunks(conf=conf):
            cols = [_deep(deep, res=0)]
            for n_ch in LEAN_CHUNKS:
                for res in (0, 9):
                    for last in (1, 16):
                        cols.append(col(lean_length(n_ch, res, last), res=res, ref="ACGT"[n_ch % 4], alts="edges",
                                        tag="n_ch=%d" % n_ch))
            cols += [col(0, tag="empty"), col(30, ref="N", alts="edges", tag="gated")]
            return edge_batch(cols, seed=500, min_bq=conf.get("min_bq", MIN_BQ), min_alt_bq=conf.get("min_alt_bq", MIN_ALT_BQ))
        t.append(Row("lean/chunks/%s" % ("one_thr" if same_thr else "two_thr"), "lean", consts, chunks, conf,
                     _kernels(deep, same_thr),
                     "chunk counts at which the lean loop's remainder, peeled trip and second trip begin, at residues 0 and 9, "
                     "last chunks of 1 and 16 observations; low qualities everywhere", {}))
    for ncols in (WG_WAVES - 1, WG_WAVES, WG_WAVES + 1):
        def sized(ncols=ncols):
            rng = np.random.default_rng(ncols)
            cols = [_deep(deep, res=0)] + [col(int(rng.integers(100, 2200)), ref="ACGT"[i % 4], alts="edges") for i in range(ncols)]
            cols[3] = col(0, tag="empty")
            cols[7] = col(40, ref="N", alts="edges", tag="gated")
            return edge_batch(cols, seed=600 + ncols)
        t.append(Row("lean/ncols%d" % ncols, "lean", consts, sized, {}, _kernels(deep, True),
                     "%d columns behind the deep one: %d columns per workgroup" % (ncols, WG_WAVES), {}))
    # the bound gate's statistic: kept rows of bq <= 31 in the whole chunks of the loop's first trip.  Rows of quality 20 in
    # the first chunk, in the last chunk and behind the first trip must not count; 63 inside it round down to 0 (the gate
    # does not fire: a DP kernel reads rows), 64 fire it
    subset = C["LFQ_BOUND_SUBSET"][0]
    for inside in (63, 64):
        def nlo(inside=inside):
            cols = []
            for c in range(24):
                res, n = (5 * c) % 16, 4203 + c
                first = 16 - res                                # observations of the first chunk
                last = (res + n - 1) % 16 + 1                   # ... of the last
                low = list(range(first)) + list(range(first + 16, first + 16 + inside)) \
                    + list(range(first + subset + 32, first + subset + 32 + 1024)) + list(range(n - last, n - 1))
                cols.append(col(n, res=res, alts=[n - 1], q=40, low=sorted(set(low)), n_every=0, tag="n_lo"))
            return edge_batch(cols, seed=700)
        t.append(Row("lean/n_lo/%d_inside" % inside, "lean", consts + ("LFQ_BOUND_SUBSET", "LFQ_BOUND_SHIFT", "LFQ_BOUND_QLO"),
                     nlo, {}, _kernels(4203, True),
                     "rows of quality 20 fill the first chunk, the last chunk and 1024 rows behind the first trip; %d lie inside it"
                     % inside, dict(rows="> 0" if inside == 63 else "== 0")))


# no tested column pruned.  Neither the library nor the oracle refuses a sig; 0.999 is the largest value at which "p * bonf < sig"
# is no rounding question for a p-value next to 1 (dp_edges / test_gpu_dp_edges.py: NO_PRUNE)
SCAN_SIG = 0.999


def scan_batch(ncols):
    """ncols columns, untested (one reference base) but for a light, a mid and a big column on each side of every tile
    edge, column 0 and the last one"""
    tested = {0: "light"}
    for edge in range(SCAN_TILE, ncols + 3, SCAN_TILE):
        for i, cls in zip(range(edge - 3, edge + 3), ("light", "mid", "big") * 2):
            if 0 <= i < ncols:
                tested.setdefault(i, cls)
    tested.setdefault(ncols - 1, "mid")
    lens = np.ones(ncols, np.int64)
    ref = np.frombuffer(b"ACGT", np.uint8)[np.arange(ncols) % 4].copy()
    cols = {i: class_column(cls, bytes([ref[i]])) for i, cls in tested.items()}
    for i, c in cols.items():
        lens[i] = len(c["nt"])
    off = np.zeros(ncols + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    ref_code = (np.arange(ncols) % 4).astype(np.uint8)
    nt = np.repeat(ref_code, lens)
    bq = np.full(n, 30, np.uint8)
    for i, c in cols.items():
        nt[int(off[i]):int(off[i + 1])] = c["nt"]
    return dict(nt=nt, bq=bq, baq=np.full(n, 255, np.uint8), mq=np.full(n, 255, np.uint8), sq=None, col_off=off,
                ref_base=ref, tested=dict(sorted(tested.items())))


def _scan_rows(t):
    for ncols in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1):
        t.append(Row("scan/ncols%d" % ncols, "scan", ("LFQ_SCAN_THREADS", "LFQ_SCAN_ITEMS"), lambda ncols=ncols: scan_batch(ncols),
                     dict(bonf_dynamic=1, sig=SCAN_SIG),
                     _kernels(de.BIG_K + 50, True),
                     "tested columns of every class on both sides of a scan tile edge (%d columns), at column 0 and at the last"
                     % SCAN_TILE, dict(scan=True)))


MANY_NCOLS = C["maxdepth grid"][0][0] * SCAN_TILE + SCAN_TILE + 1           # 1024 * 4096 + 4097
MANY_DEEPEST = 40
MANY_CUT = 200000
MANY_TAIL = 5000


def many_columns_batch(ncols=MANY_NCOLS, seed=77):
    """ncols columns of 1 to 3 observations, alt bases in about 1 % of them (half of those columns at quality 93 throughout, called at
    any Bonferroni factor, the last column among them), every 97th reference base N; the deepest column, MANY_DEEPEST
    observations, is the last one.  A column with alt bases starts with a kept reference base: were all its kept rows one
    alt allele, its p-value would be the product of their error probabilities, 10^(-sum of qualities / 10) with BAQ and MQ
    missing, whose QUAL is a whole number before it is truncated -- and then a matter of the last bit."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 4, ncols).astype(np.int64)
    lens[-1] = MANY_DEEPEST
    alt_col = rng.random(ncols) < 0.01
    alt_col[-1] = True
    lens[alt_col & (lens == 1)] = 2
    off = np.zeros(ncols + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    n = int(off[-1])
    ref_code = rng.integers(0, 4, ncols).astype(np.uint8)
    ref = np.frombuffer(b"ACGT", np.uint8)[ref_code].copy()
    ref[96::97] = ord("N")
    col_of = np.repeat(np.arange(ncols), lens)
    at = np.arange(n) - off[:-1].astype(np.int64)[col_of]           # position inside the column
    code = ref_code[col_of]
    is_alt = alt_col[col_of] & ((at == 1) | ((at > 1) & (rng.random(n) < 0.3)))
    code = np.where(is_alt, (code + rng.integers(1, 4, n).astype(np.uint8)) % 4, code).astype(np.uint8)
    lead = alt_col[col_of] & (at == 0)
    code[(rng.random(n) < 0.01) & ~lead] = 5
    bq = np.array([2, 5, 6, 20, 31, 32, 40, 40], np.uint8)[rng.integers(0, 8, n)]
    bq[lead] = 40
    hot = rng.random(ncols) < 0.5
    hot[-1] = True                      # the last column has a record
    bq[(alt_col & hot)[col_of]] = 93        # every row of it: a kept reference row of a lower quality alone explains one alt base
    nt = code | (rng.integers(0, 2, n).astype(np.uint8) << 3)
    return dict(nt=nt, bq=bq, baq=np.full(n, 255, np.uint8), mq=np.full(n, 255, np.uint8), sq=None, col_off=off, ref_base=ref)


def cut_batch(host, c0, c1):
    """columns [c0, c1) of a host batch as a batch of its own"""
    o0, o1 = int(host["col_off"][c0]), int(host["col_off"][c1])
    out = {k: (None if host.get(k) is None else host[k][o0:o1]) for k in ("nt", "bq", "baq", "mq", "sq")}
    out["col_off"] = host["col_off"][c0:c1 + 1] - np.uint64(o0)
    out["ref_base"] = host["ref_base"][c0:c1]
    for k in ("coverage_plp", "num_bases"):
        if host.get(k) is not None:
            out[k] = host[k][c0:c1]
    return out


WRAP_DEPTH = MULTI_BELOW - 1
WRAP_NCOLS = -(-2 ** 32 // WRAP_DEPTH) + 300
WRAP_SEED = 0x2F0D5EED


WRAP_PERIOD = 997


def wrap_columns():
    """the columns of the beyond-2^32 batch that are compared with the oracle: the 400 around the column whose start is
    the first at or beyond 2^32 observations, every 1000th, and every 21st of the planted ones (every WRAP_PERIOD-th column is
    planted, its allele frequency cycling through four values; the oracle takes 20 to 40 ms for one)"""
    cross = -(-2 ** 32 // WRAP_DEPTH)
    return cross, np.unique(np.concatenate([np.arange(cross - 200, cross + 200), np.arange(0, WRAP_NCOLS, 1000),
                                            np.arange(0, WRAP_NCOLS, 21 * WRAP_PERIOD)]))


def _large_rows(t):
    t.append(Row("many_columns", "many", ("maxdepth grid", "shallow workgroup cap", "shallow columns per workgroup",
                                          "LFQ_SCAN_THREADS", "LFQ_SCAN_ITEMS"), many_columns_batch, {},
                 _kernels(MANY_DEEPEST, True, routes=("dense/packed",)),
                 "%d columns: the stride loops of lfq_maxdepth_kernel (> %d x %d lanes) and of the shallow kernel (> %d workgroups "
                 "of %d columns), the carry loop of lfq_scan_sums_kernel (> %d tiles); the deepest column is the last"
                 % (MANY_NCOLS, C["maxdepth grid"][0][0], C["maxdepth grid"][0][1], C["shallow workgroup cap"][0],
                    C["shallow columns per workgroup"][0], C["LFQ_SCAN_THREADS"][0]), dict(large=True)))
    t.append(Row("beyond_2^32_observations", "wrap", ("count_multi_below",), None, {},
                 _kernels(WRAP_DEPTH, True, routes=("dense/packed",)),
                 "synth_batch(depth %d, %d columns, packed): the low word of a column's start wraps inside the shallow kernel's "
                 "32-bit relative chunk arithmetic" % (WRAP_DEPTH, WRAP_NCOLS), dict(large=True)))


def boundary_table():
    t = []
    _routing_rows(t)
    _shallow_rows(t)
    _lean_rows(t)
    _scan_rows(t)
    _large_rows(t)
    assert len({r.name for r in t}) == len(t)
    return t


def small_rows():
    return [r for r in boundary_table() if not r.checks.get("large")]
