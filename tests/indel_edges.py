"""Indel columns at the gate, packing and routing boundaries of the indel caller (lfq_indel_api.hip: lfq_call_indels_batch,
lfq_call_indel_tests_batch; lfq_pileup.hip: lfq_indel_pack_kernel; lfq_api.hip: lfq_indel_batch_device).

Used by test_indel_edges.py (CPU: every claim against the oracle's call_indels restatement, the exact tail, the oracle's pileup
and the 2.1.4 binary's VCF) and test_gpu_indel_edges.py (every row on the device, on the host-pack and the device-pack route):

  constants       the routing constants of dp_edges / count_edges (read from the sources there) and the pack kernel's geometry;
  col / ev        one column as the list of its reads: plain reads, reads that end in the column, reads with an insertion or a
                  deletion behind it -- the column dict for IndelColumns.from_columns and the reads for ReadSet.pileup_indels come
                  from that one list;
  boundary_table  the rows: name, group, column dicts, conf, claims, reads (or None), why.

A row's claims are written down from how the row was built, never by running a caller:
  tests      [(col, side, event, count, n_err_probs)] of every event that must be tested, in the reference's order
  classes    (some rows) {"light": n, "mid": n, "big": n}: the DP class of the row's tests (dp_edges.dp_class)
  kernel     (count route) the count kernel lfq_launch_count must choose, and max_col_obs
  exact      (dp route, flags) per test the levels [(rows, (sq, mq, aq, q))] of its pseudo-column, for the exact tail
  twin       (pack/bytes) the name of the row whose values are this row's after the byte clamps

No test in here."""
import os
import re
from collections import namedtuple

import mpmath
import numpy as np

import bam_records
import count_edges as ce
import dp_edges as de
import pileup_edges as pe

PLP_SRC = "lofreq_amd/csrc/lfq_pileup.hip"
API_SRC = "lofreq_amd/csrc/lfq_indel_api.hip"
USE_MQ, USE_SQ, USE_IDAQ = 2, 4, 8              # lfq_conf.flag bits (include/lofreq_amd.h); bit 1, BAQ, is not read here


def _source(path, pattern):
    """the groups of the only line of `path` that matches `pattern`"""
    with open(os.path.join(pe.ROOT, path)) as f:
        found = [m for line in f for m in [re.search(pattern, line)] if m]
    assert len(found) == 1, "%s: %d lines match %r" % (path, len(found), pattern)
    return found[0].groups()


# the pack kernel: one wavefront a test, PACK_WAVES tests a workgroup, two stride loops of PACK_LANES lanes
PACK_LANES = int(_source(PLP_SRC, r"for \(int i = lane; i < D\.ne_len; i \+= (\d+)\)")[0])
assert int(_source(PLP_SRC, r"for \(int i = lane; i < D\.rd_len; i \+= (\d+)\)")[0]) == PACK_LANES
PACK_WAVES = int(_source(PLP_SRC, r"const int64_t t = \(int64_t\)blockIdx\.x \* (\d+) \+ \(threadIdx\.x >> 6\);")[0])
POLYAT_AF = float(_source(API_SRC, r"cnt\[0\]\[i\] / denom < ([0-9.]+)f && cnt\[1\]\[i\] / denom < [0-9.]+f")[0])
Q_MAX = int(_source(API_SRC, r"return q < 0 \? \(uint8_t\)LFQ_Q_MISSING : \(uint8_t\)std::min\(q, (\d+)\);")[0])
Q_MISSING = bam_records.source_constant("LFQ_Q_MISSING", "include/lofreq_amd.h")
MQ0_P = float(_source("lofreq_amd/csrc/lfq_api.hip", r"L->mq\[0\] = ([0-9.]+);")[0])
LENGTHS = (0, 1, PACK_LANES - 1, PACK_LANES, PACK_LANES + 1, 2 * PACK_LANES, 2 * PACK_LANES + 1)
MIN_COV = 10                                    # the conf of the groups `gates` and `poly-AT` (-C 10 for the binary)

Row = namedtuple("Row", "name group cols conf claim reads why")


# ---- one column as the list of its reads -----------------------------------------------------------------------------------

SLOT, P = 48, 10                                # a column of a `reads` row sits at position P of a slot of SLOT reference bases
HEAD = "GCTGACGTCA"
TAIL = "GCAGTCAGTGCTAGCATCGATGCATGCTAGTCGATCAGCTAGCTA"


def _val(v, i, j):
    """a number, a function of the read's index i in its column, or a list over the reads of its kind or event (the last entry
    for every further read)"""
    if callable(v):
        return int(v(i))
    if isinstance(v, (list, tuple)):
        return int(v[min(j, len(v) - 1)])
    return int(v)


def ev(key, n, q=40, aq=50, mq=60, sq=-1):
    """an event carried by n reads; q, aq, mq, sq: see _val"""
    return dict(key=key, n=n, q=q, aq=aq, mq=mq, sq=sq)


def col(plain=0, tails=0, ins=(), dels=(), ref="C", q=40, mq=60, rev=lambda i: i % 3 == 1):
    """a column as its reads in pileup order: `plain` reads through it, `tails` reads that end in it, the reads of the insertion
    events, the reads of the deletion events.  A read has one indel quality q (its BI and BD), a mapping quality, a strand and,
    with an event, an alignment quality (its ai and ad) and a source quality"""
    reads = []

    def add(kind, key, j, q_, aq_, mq_, sq_):
        i = len(reads)
        reads.append(dict(kind=kind, key=key, q=_val(q_, i, j), aq=_val(aq_, i, j), mq=_val(mq_, i, j), sq=_val(sq_, i, j),
                          rev=bool(rev(i))))
    for j in range(plain):
        add("plain", None, j, q, -1, mq, -1)
    for j in range(tails):
        add("tail", None, plain + j, q, -1, mq, -1)
    for kind, events in (("ins", ins), ("del", dels)):
        for e in events:
            for j in range(e["n"]):
                add(kind, e["key"], j, e["q"], e["aq"], e["mq"], e["sq"])
    return dict(ref=ref, reads=reads)


def slot_ref(spec, for_reads=True):
    """the slot's reference: the column's base at P, the deleted bases behind it (for reads, the keys of a column's deletions are
    prefixes of one another)"""
    keys = [r["key"] for r in spec["reads"] if r["kind"] == "del"]
    longest = max(keys, key=len) if keys else ""
    assert not for_reads or (all(longest.startswith(k) for k in keys) and len(longest) <= SLOT - P - 8), keys
    return (HEAD + spec["ref"] + longest + TAIL)[:SLOT]


def hrun_of(ref, pos):
    """get_hrun (plp.c:751-787): the run of ref[pos + 1] to the right of pos + 1 and to the left from pos"""
    if pos + 1 >= len(ref):
        return 1
    c, n = ref[pos + 1].upper(), 1
    i = pos + 2
    while i < len(ref) and ref[i].upper() == c:
        n, i = n + 1, i + 1
    i = pos
    while i >= 0 and ref[i].upper() == c:
        n, i = n + 1, i - 1
    return n


def column_dict(spec, hrun):
    """the column for IndelColumns.from_columns (compile_plp_col's indel part, plp.c:1019-1192): a read without an event of a
    side is a non-event read of that side"""
    reads = spec["reads"]
    d = {"ref": spec["ref"], "coverage_plp": len(reads), "num_tails": sum(r["kind"] == "tail" for r in reads),
         "num_non_indels": sum(r["kind"] in ("plain", "tail") for r in reads), "hrun": hrun}
    for sn, kind in (("ins", "ins"), ("dels", "del")):
        non = [r for r in reads if r["kind"] != kind]
        events = {}
        for r in reads:
            if r["kind"] == kind:
                events.setdefault(r["key"], []).append(r)
        d[sn] = {"non_fw": sum(not r["rev"] for r in non), "non_rv": sum(r["rev"] for r in non),
                 "ne_q": [r["q"] for r in non], "ne_mq": [r["mq"] for r in non],
                 "events": [{"key": k, "fw": sum(not r["rev"] for r in rs), "rv": sum(r["rev"] for r in rs),
                             "q": [r["q"] for r in rs], "aq": [r["aq"] for r in rs], "mq": [r["mq"] for r in rs],
                             "sq": [r["sq"] for r in rs]} for k, rs in events.items()]}
    return d


def _pileup_read(pos0, cigar, seq, r):
    assert 0 <= r["q"] <= 93 and 0 <= r["mq"] <= 255 and -1 <= r["aq"] <= 93 and r["sq"] == -1, r
    ql = len(seq)
    tag = lambda v: None if v < 0 else np.full(ql, 33 + v, np.uint8)
    aq = r["aq"] if r["key"] else 50          # a read without an event carries the tags too: nothing reads them in its column
    return {"pos0": pos0, "cigar": pe.parse(cigar), "seq": np.array(["ACGT".find(c) % 5 for c in seq], np.uint8),
            "qual": np.full(ql, 30, np.uint8), "mapq": r["mq"], "reverse": r["rev"], "lb": np.full(ql, 33 + 40, np.uint8),
            "bi": tag(r["q"]), "bd": tag(r["q"]), "ai": tag(aq), "ad": tag(aq)}


def slot_reads(spec, ref, off):
    """the reads of a column whose slot starts at `off` of the reference `ref`: all start five bases before the column"""
    p = off + P
    out = []
    for r in spec["reads"]:
        if r["kind"] == "plain":
            out.append(_pileup_read(p - 5, "12M", ref[p - 5:p + 7], r))
        elif r["kind"] == "tail":
            out.append(_pileup_read(p - 5, "6M", ref[p - 5:p + 1], r))
        elif r["kind"] == "ins":
            k = r["key"]
            out.append(_pileup_read(p - 5, "6M%dI6M" % len(k), ref[p - 5:p + 1] + k + ref[p + 1:p + 7], r))
        else:
            n = len(r["key"])
            assert ref[p + 1:p + 1 + n] == r["key"]
            out.append(_pileup_read(p - 5, "6M%dD6M" % n, ref[p - 5:p + 1] + ref[p + 1 + n:p + 7 + n], r))
    return out


def n_tests_of(cols, tested):
    """(col, side, event) -> (col, side, event, count, n_err_probs): the event's reads, and every read of the side's lists"""
    out = []
    for c, sd, e in tested:
        s = cols[c][("ins", "dels")[sd]]
        first = sum(len(cols[k].get(("ins", "dels")[sd], {}).get("events", [])) for k in range(c))
        out.append((c, sd, first + e, len(s["events"][e]["q"]), len(s["ne_q"]) + sum(len(x["q"]) for x in s["events"])))
    return out


def _add(t, name, group, specs, tested, conf=None, over=None, reads=True, why="", **claim):
    """specs: col(...) per column; tested: [(col, side, event of the column's side)]; over(cols): changes to the column dicts
    that no read could produce (the row is then a from_columns row only)"""
    ref = "".join(slot_ref(s, reads and not over) for s in specs)
    cols = [column_dict(s, hrun_of(ref, i * SLOT + P)) for i, s in enumerate(specs)]
    rd = None
    if over:
        over(cols)
    elif reads:
        rd = dict(reads=[r for i, s in enumerate(specs) for r in slot_reads(s, ref, i * SLOT)], ref=ref,
                  pos=[i * SLOT + P for i in range(len(specs))])
    t.append(Row(group + "/" + name, group, cols, dict(conf or {}), dict(claim, tests=n_tests_of(cols, tested)), rd, why))


def all_events(specs):
    """every event of every column, in the reference's order: insertions first"""
    out = []
    for c, s in enumerate(specs):
        for sd, kind in enumerate(("ins", "del")):
            keys = []
            for r in s["reads"]:
                if r["kind"] == kind and r["key"] not in keys:
                    keys.append(r["key"])
            out += [(c, sd, e) for e in range(len(keys))]
    return out


# ---- gates -------------------------------------------------------------------------------------------------------------------

def _gate_rows(t):
    conf = dict(min_cov=MIN_COV)
    std = lambda **kw: col(plain=kw.pop("plain", 20), ins=[ev("G", 4)], dels=[ev("A", 3)], **kw)
    both = [(0, 0, 0), (0, 1, 0)]
    _add(t, "ref_N", "gates", [std(ref="N")], [], conf, why="lofreq_call.c:892: no test on a reference N")
    _add(t, "ref_A", "gates", [std(ref="A")], both, conf, why="... and both tests on any other base")

    def lower_n(cols):
        cols[0]["ref"] = "n"
    _add(t, "ref_lower_n", "gates", [std()], both, conf, over=lower_n, why="the gate compares with 'N' only")
    _add(t, "min_cov/sum_equal", "gates", [std(plain=MIN_COV - 7)], both, conf, why="num_non_indels + num_ins + num_dels == min_cov")
    _add(t, "min_cov/sum_below", "gates", [std(plain=MIN_COV - 8)], [], conf, why="the sum one below min_cov")

    def cov(v):
        def f(cols):
            cols[0]["coverage_plp"] = v
        return f
    _add(t, "min_cov/coverage_above_sum_below", "gates", [std(plain=MIN_COV - 8)], [], conf, over=cov(MIN_COV + 2),
         why="coverage_plp >= min_cov, the sum below it: the gate reads the sum (:626)")
    _add(t, "min_cov/coverage_below_sum_equal", "gates", [std(plain=MIN_COV - 7)], both, conf, over=cov(MIN_COV - 2),
         why="coverage_plp < min_cov, the sum at it")

    def zero(k):
        def f(cols):
            cols[0][k] = 0
        return f
    _add(t, "num_ins_zero", "gates", [std()], [(0, 1, 0)], conf, over=zero("num_ins"), why="num_ins == 0 with insertions listed (:684)")
    _add(t, "num_dels_zero", "gates", [std()], [(0, 0, 0)], conf, over=zero("num_dels"), why="num_dels == 0 with deletions listed (:706)")
    _add(t, "ins_only", "gates", [col(plain=20, ins=[ev("G", 4), ev("GT", 2)])], [(0, 0, 0), (0, 0, 1)], conf, why="no deletion side")
    _add(t, "dels_only", "gates", [col(plain=20, dels=[ev("A", 4), ev("AT", 2)])], [(0, 1, 0), (0, 1, 1)], conf, why="no insertion side")


# ---- poly-AT -----------------------------------------------------------------------------------------------------------------

def _pair(key, n_ins, n_del, denom, tails=0, extra_ins=()):
    """an insertion and a deletion of `key` on n_ins and n_del of the denom + tails reads of a column"""
    n_extra = sum(e["n"] for e in extra_ins)
    return col(plain=denom - n_ins - n_del - n_extra, tails=tails, ins=[ev(key, n_ins)] + list(extra_ins), dels=[ev(key, n_del)])


def _polyat_rows(t):
    """lofreq_call.c:649-681: a 1-bp A or T insertion AND deletion in one column, both with count / (coverage_plp - num_tails)
    below 0.05f in float arithmetic, are not tested.  5 / 100, 1 / 20 and 50 / 1000 round to the float 0.05f itself, which is
    not below it: tested.  (In double, 0.05 < (double)0.05f: ignored.)"""
    assert POLYAT_AF == 0.05
    conf = dict(min_cov=MIN_COV)
    both, none = [(0, 0, 0), (0, 1, 0)], []
    for cnt, denom, tested in ((4, 100, none), (5, 100, both), (1, 20, both), (50, 1000, both), (49, 1000, none), (3, 61, none)):
        f = np.float32(cnt) / np.float32(denom)
        assert (f < np.float32(0.05)) == (tested is none)
        _add(t, "line/%d_of_%d" % (cnt, denom), "poly-AT", [_pair("A", cnt, cnt, denom)], tested, conf,
             why="count / denom = %d / %d: %s 0.05f in float" % (cnt, denom, "below" if tested is none else "at"))
    _add(t, "only_ins_below", "poly-AT", [_pair("A", 4, 6, 100)], both, conf, why="the deletion at 6 / 100: both tested")
    _add(t, "only_del_below", "poly-AT", [_pair("T", 6, 4, 100)], both, conf, why="the insertion at 6 / 100: both tested")
    _add(t, "tails/105_5", "poly-AT", [_pair("A", 5, 5, 100, tails=5)], both, conf,
         why="coverage_plp 105, num_tails 5: 5 / 100 is on the line (5 / 105 would be below it)")
    _add(t, "tails/104_5", "poly-AT", [_pair("A", 5, 5, 99, tails=5)], both, conf, why="coverage_plp 104, num_tails 5: 5 / 99")
    _add(t, "tails/85_5", "poly-AT", [_pair("A", 4, 4, 80, tails=5)], both, conf,
         why="4 / 80 is on the line (4 / 85 would be below it)")
    keys = ("A", "T", "C", "G", "AA", "AT")
    _add(t, "keys", "poly-AT", [_pair(k, 4, 4, 100) for k in keys],
         [(c, sd, 0) for c, k in enumerate(keys) if k not in ("A", "T") for sd in (0, 1)], conf,
         why="the rule is for the keys A and T alone; C, G, AA, AT at 4 / 100 are tested")
    # (two deletions of one base have one key in a pileup: from_columns only)
    two = col(plain=100 - 18, ins=[ev("A", 4), ev("T", 4)], dels=[ev("A", 4), ev("T", 6)])
    _add(t, "A_pair_and_T_pair", "poly-AT", [two], [(0, 0, 1), (0, 1, 1)], conf, reads=False,
         why="A: both below, ignored; T: the deletion at 6 / 100, both tested")

    def no_ne(sn):
        def f(cols):
            cols[0][sn]["ne_q"], cols[0][sn]["ne_mq"] = [], []
        return f
    _add(t, "ne_ins_zero", "poly-AT", [_pair("A", 4, 4, 100)], both, conf, over=no_ne("ins"),
         why="no read without an insertion: the rule is off (:650), both tested")
    _add(t, "ne_del_zero", "poly-AT", [_pair("A", 4, 4, 100)], both, conf, over=no_ne("dels"), why="... without a deletion")
    _add(t, "ignored_A_beside_AT", "poly-AT", [_pair("A", 4, 4, 100, extra_ins=[ev("AT", 4)])], [(0, 0, 1)], conf,
         why="the A pair is ignored, the AT insertion tested over all 100 reads, the ignored insertion's among them; one test counted")


# ---- pack --------------------------------------------------------------------------------------------------------------------

# qualities that differ from read to read: a row written to another read's place changes the p-value
_AQ = lambda i: 5 + i % 30
_MQ = lambda i: 20 + (i * 3) % 40


def _q(base):
    return lambda i: base + (i * 5) % 7


def _vev(key, n, base=3):
    return ev(key, n, q=_q(base), aq=_AQ, mq=_MQ)


def _vcol(plain, base=3, **kw):
    return col(plain=plain, q=_q(base), mq=_MQ, **kw)


def _pack_rows(t):
    conf = dict(flag=USE_MQ | USE_IDAQ)
    specs = []
    for i, ne in enumerate(LENGTHS):
        for j, rd in enumerate(LENGTHS):
            if rd:                  # (a tested event has a read: rd_len >= 1)
                base = dp_quality(rd, ne + rd)          # about rd errors expected: no p-value next to 1
                specs.append(_vcol(ne, base, ins=[_vev("G", rd, base)]) if (i + j) % 2 == 0 else
                             _vcol(ne, base, dels=[_vev("AT", rd, base)]))
    _add(t, "lengths", "pack", specs, all_events(specs), conf,
         why="ne_len x rd_len over %s, insertion and deletion side in turn; me_len == rd_len" % (LENGTHS,))
    three = [_vcol(7, ins=[_vev("G", a), _vev("GT", b), _vev("C", c)], dels=[_vev("A", c), _vev("AT", a), _vev("ATG", b)])
             for a, b, c in ((1, 5, 7), (5, 1, 7), (5, 7, 1))]
    _add(t, "three_events", "pack", three, all_events(three), conf, why="the event of me_len 1 first, middle and last of three")
    for n in (1, PACK_WAVES - 1, PACK_WAVES, PACK_WAVES + 1, 2 * PACK_WAVES, 2 * PACK_WAVES + 1):
        specs = [_vcol(5 + c, ins=[_vev("G", 2)]) for c in range(n)]
        _add(t, "tests/%d" % n, "pack", specs, all_events(specs), conf, why="%d tests: %d to a workgroup" % (n, PACK_WAVES))
    for first, second in ((17, 15), (17, 16), (17, 30)):
        specs = [_vcol(first - 2, ins=[_vev("G", 2)]), _vcol(second - 3, dels=[_vev("A", 3)])]
        _add(t, "observations/%d" % (first + second), "pack", specs, all_events(specs), conf,
             why="%d observations in all, %d mod 16; the second test starts at %d" % (first + second, (first + second) % 16, first))
    # byte values no read gives (a BI / BD byte is 33 .. 126, an ai / ad byte too): from_columns only.  The twin row holds the
    # values the clamps must make of them.  A quality below 0 becomes 0, an error probability of 1; no pseudo-column here has
    # two such rows (the reference's recurrence has no answer for two certain errors: inf - inf)
    big = [Q_MAX, Q_MAX + 1, 300]
    all_flags = dict(flag=USE_MQ | USE_SQ | USE_IDAQ)

    def bytes_cols(clamp):
        c = (lambda v: [min(max(x, 0), Q_MAX) for x in v]) if clamp else (lambda v: v)          # the bq clamp
        c8 = (lambda v: [-1 if x < 0 else min(x, Q_MAX) for x in v]) if clamp else (lambda v: v)  # q8 / lfq_q8
        d = lambda: [ev("A", 3, q=30, aq=40, mq=60, sq=35)]
        return [
            col(plain=10, q=c([-5] + big + [30]), mq=60, ins=[ev("G", 5, q=c(big + [30]), aq=40, mq=60, sq=35)], dels=d()),
            col(plain=10, q=c([0, 30]), mq=60, ins=[ev("G", 5, q=c(big[::-1] + [30]), aq=40, mq=60, sq=35)], dels=d()),
            col(plain=10, q=30, mq=60, ins=[ev("G", 5, q=c([30, -5, 30]), aq=40, mq=60, sq=35)], dels=d()),
            col(plain=10, q=30, mq=60, ins=[ev("G", 7, q=30, aq=c8([-1, 0] + big + [40]), mq=60, sq=35), ev("C", 2, q=30)], dels=d()),
            col(plain=10, q=30, mq=60, ins=[ev("G", 7, q=30, aq=40, mq=60, sq=c8([-1, 0] + big + [40]))], dels=d()),
            col(plain=10, q=30, mq=c8([-1, 0, Q_MAX, 300, 60]), ins=[ev("G", 7, q=30, aq=40, mq=c8([-1, 0, Q_MAX, 300, 60]), sq=35)],
                dels=d()),
        ]
    for name, clamp, twin in (("raw", False, "pack/bytes/clamped"), ("clamped", True, None)):
        specs = bytes_cols(clamp)
        _add(t, "bytes/" + name, "pack", specs, all_events(specs), all_flags, reads=False, twin=twin,
             why="q -5 / %d / 300 -> 0 / %d / %d; aq, mq, sq -1 -> missing, %d / 300 -> %d" % (Q_MAX + 1, Q_MAX, Q_MAX, Q_MAX + 1, Q_MAX))
    cyc = lambda v: (lambda i: v[i % len(v)])
    # mapping quality 255: missing on a read with an event (snpcaller.c:544), used as it stands on one without (:523-526)
    m255 = col(plain=14, q=30, mq=cyc([255, 60]), ins=[ev("G", 6, q=30, mq=cyc([255, 60, 255]))], dels=[ev("A", 4, q=30, mq=255)])
    _add(t, "bytes/mq255", "pack", [m255], all_events([m255]), dict(flag=USE_MQ), reads=False,
         why="mapping quality 255 on reads with and without an event")


# ---- flags -------------------------------------------------------------------------------------------------------------------

FLAGS = (0, USE_MQ, USE_SQ, USE_IDAQ, USE_MQ | USE_SQ | USE_IDAQ)
FLAGS_AQ, FLAGS_Q, FLAGS_MQ, FLAGS_SQ = 1, 40, 60, 25


def _levels(reads, kind, key, flag):
    """the pseudo-column of the event `key` as [(rows, (sq, mq, aq, q))]: what plp_to_ins_errprobs / plp_to_del_errprobs
    (snpcaller.c:502-623) merge for each read -- the alignment quality on the tested event's reads alone"""
    out = {}
    for r in reads:
        event = r["kind"] == kind
        mq = r["mq"] if flag & USE_MQ else -1
        if event and mq == 255:
            mq = -1
        lv = (r["sq"] if event and flag & USE_SQ else -1, mq, r["aq"] if event and r["key"] == key and flag & USE_IDAQ else -1,
              r["q"])
        out[lv] = out.get(lv, 0) + 1
    return [(n, lv) for lv, n in out.items()]


def _exact_of(specs, tested, flag):
    out = []
    for c, sd, e in tested:
        kind = ("ins", "del")[sd]
        keys = []
        for r in specs[c]["reads"]:
            if r["kind"] == kind and r["key"] not in keys:
                keys.append(r["key"])
        out.append(_levels(specs[c]["reads"], kind, keys[e], flag))
    return out


def _flag_rows(t):
    for flag in FLAGS:
        for name, sq in (("columns", FLAGS_SQ), ("reads", -1)):
            e = lambda key: ev(key, 3, q=FLAGS_Q, aq=FLAGS_AQ, mq=FLAGS_MQ, sq=sq)
            spec = col(plain=30, q=FLAGS_Q, mq=FLAGS_MQ, ins=[e("G"), e("GT"), e("C")], dels=[e("A"), e("AT"), e("ATG")])
            tested = all_events([spec])
            _add(t, "%s/flag%d" % (name, flag), "flags", [spec], tested, dict(flag=flag), reads=name == "reads",
                 exact=_exact_of([spec], tested, flag),
                 why="three events a side, alignment quality %d on every event read: it belongs to the tested event alone "
                     "(snpcaller.c:537)" % FLAGS_AQ)


# ---- count route -------------------------------------------------------------------------------------------------------------

def _count_rows(t):
    for n in (ce.LPG4_BELOW, ce.LPG4_BELOW + 1, ce.LPG8_BELOW, ce.LPG8_BELOW + 1, ce.MULTI_BELOW - 1, ce.MULTI_BELOW):
        for flag in (USE_MQ | USE_IDAQ, USE_MQ | USE_IDAQ | USE_SQ):
            specs = [_vcol(20, ins=[_vev("G", 3)]), col(plain=n - 4, q=40, mq=_MQ, ins=[ev("G", 4, q=40, aq=_AQ, mq=_MQ, sq=30)]),
                     _vcol(33, dels=[_vev("A", 2)])]
            _add(t, "%d/flag%d" % (n, flag), "count route", specs, all_events(specs), dict(flag=flag), reads=False, max_col_obs=n,
                 kernel=ce.expected_kernel(n, packed=False, dense_strand=True, same_thr=True),
                 why="the deepest pseudo-column has %d observations; byte nt, dense strand counts, min_bq = min_alt_bq = 0, an sq "
                     "track" % n)


# ---- dp route ----------------------------------------------------------------------------------------------------------------

def dp_boundaries():
    """(boundary, k, n, class): the tested event's read count and the pseudo-column's depth on each side of every light / mid /
    big boundary dp_edges.dp_class knows, and around the screen variants' MAXK; n the smallest depth of the class (with one
    read that has no event)"""
    out = []

    def add(boundary, k, n, cls):
        assert de.dp_class(k, n) == cls and n > k, (boundary, k, n, cls)
        if (k, n) not in [(x[1], x[2]) for x in out]:         # (MAXK = 11 meets the suspicious floor)
            out.append((boundary, k, n, cls))
    k = de.MID_K - 1
    add("suspicious at MID_K - 1", k, de.light_min_n(k), "light")
    add("suspicious at MID_K - 1", k, de.light_min_n(k) - 1, "mid")
    add("K = MID_K", de.MID_K, de.MID_K + 1, "mid")
    add("suspicious floor", de.SUSP_FLOOR - 1, de.SUSP_FLOOR, "light")
    add("suspicious floor", de.SUSP_FLOOR, de.SUSP_FLOOR + 1, "mid")
    for k in (de.SUSP_FLOOR, de.SUSP_FLOOR + 1):
        add("suspicious above the floor", k, de.light_min_n(k), "light")
        add("suspicious above the floor", k, de.light_min_n(k) - 1, "mid")
    add("K = BIG_K - 1", de.BIG_K - 1, de.BIG_K, "mid")
    add("K = BIG_K", de.BIG_K, de.BIG_K + 1, "big")
    for maxk in de.SCREEN_MAXK:
        for k in (maxk - 1, maxk, maxk + 1):
            add("screen MAXK = %d" % maxk, k, max(de.light_min_n(k), k + 1), "light")
    return out


def dp_quality(k, n):
    """the quality at which k of n rows is about the mean: a p-value neither next to 1 nor deep"""
    return int(min(40, max(3, round(-10 * np.log10(k / n)))))


def _dp_rows(t):
    for boundary, k, n, cls in dp_boundaries():
        q = dp_quality(k, n)
        for flag, aq in ((0, -1), (USE_IDAQ, q + 2)):
            spec = col(plain=n - k, q=q, mq=60, ins=[ev("G", k, q=q, aq=aq, mq=60)])
            _add(t, "k%d/n%d/flag%d" % (k, n, flag), "dp route", [spec], [(0, 0, 0)], dict(flag=flag), reads=False,
                 classes={c: int(c == cls) for c in ("light", "mid", "big")}, exact=_exact_of([spec], [(0, 0, 0)], flag),
                 why="%s: k = %d, n = %d is %s; quality %d%s" % (boundary, k, n, cls, q,
                                                                  ", alignment quality %d on the event's rows" % aq if flag else ""))


# ---- state -------------------------------------------------------------------------------------------------------------------

def _state_rows(t):
    a = [col(plain=60 + 7 * c, q=30, ins=[ev("G", 1 + c % 3, q=30)], dels=[ev("A", 1 + (c + 1) % 3, q=30)]) for c in range(12)]
    ks = (1, 5, 12, 23, 40, 31, 2)
    b = [col(plain=max(de.light_min_n(k), 50) - k, q=dp_quality(k, max(de.light_min_n(k), 50)), ins=[ev("G", k, q=20)]) for k in ks]
    for name, specs in (("A", a), ("B", b)):
        tested = all_events(specs)
        kmax = max(n for _, _, _, n, _ in n_tests_of([column_dict(s, 1) for s in specs], tested))
        classes = {"light": len(tested), "mid": 0, "big": 0}
        _add(t, name, "state", specs, tested, dict(flag=USE_MQ), reads=False, classes=classes, kmax=kmax,
             why="every tested event has at most %d reads; all light: the K histogram of this batch sets the next batch's screen "
                 "variant" % kmax)


# ---- wide --------------------------------------------------------------------------------------------------------------------

WIDE_N = 400001
WIDE_PARTS = (2, 3, 4)


def wide_positions():
    """the first column of every part of a scan over WIDE_N columns split in 2, 3 or 4, and the column before it"""
    return sorted({WIDE_N * p // parts - d for parts in WIDE_PARTS for p in range(1, parts) for d in (0, 1)})


def _wide_row(t):
    """every position of the region under one background read (reads of 100 bases end to end), and at each part boundary a
    cluster of reads that start six bases before it: some with an insertion behind the last column of a part, some with one
    behind the first column of the next"""
    ref = pe.make_ref(WIDE_N + 120, 41)
    pos = wide_positions()
    firsts = sorted(set(pos[1::2]))
    assert len(pos) == 2 * len(firsts) and all(p - 1 in pos for p in firsts)
    bg_q, bg_mq = 35, 50
    starts = [0] + list(range(150, WIDE_N, 100))
    lens = [150] + [100] * (len(starts) - 1)
    assert all((s + l - 1) not in pos for s, l in zip(starts, lens)) and starts[-1] + lens[-1] >= WIDE_N
    bg = dict(kind="plain", key=None, q=bg_q, aq=-1, mq=bg_mq, sq=-1, rev=False)
    reads = [(s, _pileup_read(s, "%dM" % l, ref[s:s + l], bg)) for s, l in zip(starts, lens)]
    cols = []
    for k, p in enumerate(firsts):
        n_plain, n_a, n_b = 6 + k, 3 + k % 2, 4
        cl = col(plain=n_plain, q=30, mq=60, ins=[ev("G", n_a, q=25 + k, aq=40), ev("TC", n_b, q=28, aq=45 - k)])
        for r in cl["reads"]:
            if r["kind"] == "plain":
                reads.append((p - 6, _pileup_read(p - 6, "12M", ref[p - 6:p + 6], r)))
            elif r["key"] == "G":                         # behind position p - 1
                reads.append((p - 6, _pileup_read(p - 6, "6M1I6M", ref[p - 6:p] + "G" + ref[p:p + 6], r)))
            else:                                         # behind position p
                reads.append((p - 6, _pileup_read(p - 6, "7M2I5M", ref[p - 6:p + 1] + "TC" + ref[p + 1:p + 6], r)))
        # the background read starts before the cluster: it is the first read of both columns
        for at, key in ((p - 1, "G"), (p, "TC")):
            seen = dict(ref=ref[at], reads=[bg] + [dict(r, kind="plain" if r["key"] != key else "ins") for r in cl["reads"]])
            cols.append(column_dict(seen, hrun_of(ref, at)))
    reads.sort(key=lambda x: x[0])
    rd = dict(reads=[r for _, r in reads], ref=ref, pos=pos, end=WIDE_N)
    tested = [(c, 0, 0) for c in range(len(cols))]
    t.append(Row("wide/part_boundaries", "wide", cols, dict(flag=USE_MQ | USE_IDAQ), dict(tests=n_tests_of(cols, tested)), rd,
                 "%d columns: the column scan of lfq_call_indels_batch runs on threads; an event in the last column of a part and in "
                 "the first of the next, for 2, 3 and 4 parts" % WIDE_N))


def boundary_table():
    t = []
    _gate_rows(t)
    _polyat_rows(t)
    _pack_rows(t)
    _flag_rows(t)
    _count_rows(t)
    _dp_rows(t)
    _state_rows(t)
    _wide_row(t)
    assert len({r.name for r in t}) == len(t)
    return t


_TABLE = []


def table():
    """boundary_table(), built once"""
    if not _TABLE:
        _TABLE.extend(boundary_table())
    return _TABLE


def golden_rows():
    """the `reads` rows of the groups gates and poly-AT: what tests/make_indel_edges_golden.py hands the 2.1.4 binary"""
    return [r for r in table() if r.group in ("gates", "poly-AT") and r.reads]


def golden_contig():
    """the golden rows on one contig, one behind the other -> (reference, reads, [(row name, first position, behind the last)])"""
    ref, reads, spans = "", [], []
    for r in golden_rows():
        off = len(ref)
        reads += [dict(x, pos0=x["pos0"] + off) for x in r.reads["reads"]]
        ref += r.reads["ref"]
        spans.append((r.name, off, len(ref)))
    return ref, reads, spans


# ---- the exact tail ----------------------------------------------------------------------------------------------------------

def merged_p(sq, mq, aq, q):
    """merge_srcq_mapq_baq_and_bq (snpcaller.c:303-341) in mpmath, from the doubles the quality LUT holds"""
    p = lambda v: mpmath.mpf(0) if v == -1 else mpmath.mpf(de.lut_p(v))
    mp_ = mpmath.mpf(0) if mq == -1 else mpmath.mpf(MQ0_P) if mq == 0 else mpmath.mpf(de.lut_p(mq))
    sp, bap, bp = p(sq), p(aq), p(q)
    return mp_ + (1 - mp_) * sp + (1 - mp_) * (1 - sp) * bap + (1 - mp_) * (1 - sp) * (1 - bap) * bp


def exact_log_tail(k, levels):
    """log P(X >= k) of a pseudo-column given as [(rows, (sq, mq, aq, q))]: the level with most rows is the binomial body of
    dp_edges.exact_tail, the others its further levels"""
    with mpmath.workdps(de.DPS):
        lv = sorted(levels, key=lambda x: -x[0])
        n = sum(r for r, _ in lv)
        spec = dict(n=n, p=merged_p(*lv[0][1]), levels=[(r, merged_p(*q)) for r, q in lv[1:]])
        return float(mpmath.log(de.exact_tail(k, spec)))
