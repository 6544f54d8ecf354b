"""Tiny read sets on the constants of lfq_plp_summary_kernel (lfq_pileup.hip) and on the branches of compile_plp_col that decide
plp_summary's header line (plp.c:797-1288, lofreq_call.c:445-459).

Used by test_plpsummary_edges_ref.py (CPU: every expected line below is what the restatement tests/plpsummary_ref.py gives, and
every branch of BRANCHES has a row) and by test_gpu_plpsummary.py (the kernel and the host layer against the same lines).

A Row holds the reads (dicts as lofreq_amd.ReadSet takes them, in pileup order), the contig, the region, the three options, the
branches it stands for, `expect` = {pos0: the header line of that column, written down in EXPECT below} and `ordered`: "some" =
at least one column of the call must take the kernel's ordered path, "none" = no column may, None = not stated.
"""
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHROM = "edge"
REF = "ACGTTGCAAGCTTAGGCATCGATCGGATTACAGCTAGCTAGGATCCAGTCAGCTAGCATCG"
SEQ_LETTERS = "ACGTN=MRSVWYHKDB"

Row = namedtuple("Row", "name branches reads ref begin end min_plp_bq min_plp_idq max_depth expect ordered")

# every branch the table must cover at least once (test_plpsummary_edges_ref.py)
BRANCHES = (
    "window 63", "window 64", "window 65", "window 128", "window 129",
    "only D entries", "all below min_plp_bq", "DBL_MIN increment", "quality 93", "quality 94", "quality 120",
    "N base", "IUPAC code", "N loses a tie", "exact tie", "near tie C", "near tie A", "clear winner",
    "leading S", "trailing S", "ends in I", "starts with D", "one-base read", "refskip spans",
    "insertion wins", "deletion wins", "event equals non-event", "two events tie", "insertion before deletion", "min_plp_idq decides",
    "region cut", "empty region", "max_depth drops",
)


def wave_rounds():
    """the kernel's round width, read from the source: lanes are reads, 64 per round"""
    src = open(os.path.join(ROOT, "lofreq_amd", "csrc", "lfq_pileup.hip")).read()
    body = src[src.index("void lfq_plp_summary_kernel("):]
    m = re.search(r"for \(int64_t r0 = lo; r0 < hi; r0 \+= (\d+)\)", body)
    return int(m.group(1))


def rd(pos0, cigar, seq, quals, rev=False, mapq=60, bi=None, bd=None):
    cig = [(op, int(n)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    seq = np.array([SEQ_LETTERS.index(c) for c in seq], np.uint8)
    if isinstance(quals, int):
        quals = [quals] * len(seq)
    assert len(quals) == len(seq) == sum(l for op, l in cig if op in "MIS=X")
    tag = lambda t: None if t is None else np.array([q + 33 for q in ([t] * len(seq) if isinstance(t, int) else t)], np.uint8)
    return {"pos0": pos0, "cigar": cig, "seq": seq, "qual": np.array(quals, np.uint8), "mapq": mapq, "reverse": rev,
            "bi": tag(bi), "bd": tag(bd)}


def one(p, base, q, rev=False, **kw):
    """a read of one base at p"""
    return rd(p, "1M", base, [q], rev, **kw)


def window_reads(n, p=20):
    """n reads of five bases that all cover p, sorted by start; base, quality and strand change from read to read, so that a
    wrong rank or a dropped round shows in the counts"""
    reads = []
    for i in range(n):
        start = p - 4 + (i * 5) // n                     # non-decreasing: p - 4 .. p
        seq = "".join("ACGT"[(i * 7 + j) % 4] for j in range(5))
        reads.append(rd(start, "5M", seq, [(i * 13 + j * 3) % 40 + 2 for j in range(5)], rev=i % 3 == 0))
    return reads


def table():
    W = wave_rounds()
    rows = []

    def add(name, branches, reads, begin=0, end=len(REF), bq=3, idq=0, depth=None, ordered=None):
        rows.append(Row(name, tuple(branches), reads, REF, begin, end, bq, idq, depth, EXPECT[name], ordered))

    for n in (W - 1, W, W + 1, 2 * W, 2 * W + 1):
        add("window_%d" % n, ["window %d" % n], window_reads(n))
    add("only_d", ["only D entries"], [rd(10, "3M2D3M", "GCTGGC", 30)])
    add("below_bq", ["all below min_plp_bq"], [one(12, "T", 2), one(12, "G", 1, True), one(12, "T", 0)])
    add("q0_dbl_min", ["DBL_MIN increment"], [one(12, "C", 0), one(12, "C", 0, True)], bq=0, ordered="none")
    add("cap_93_120", ["quality 93", "quality 120", "exact tie"], [one(12, "A", 93), one(12, "T", 120)], ordered="some")
    add("cap_93_94", ["quality 94"], [one(12, "C", 94), one(12, "A", 93, True)], ordered="some")
    add("n_and_iupac", ["N base", "IUPAC code", "N loses a tie"],
        [one(12, "N", 30), one(12, "R", 30, True), one(12, "T", 30), one(12, "T", 30),
         one(13, "N", 30), one(13, "Y", 20)], ordered="some")
    add("exact_tie", ["exact tie"], [one(12, "A", 11), one(12, "C", 11), one(12, "A", 37, True), one(12, "C", 37, True)],
        ordered="some")
    add("near_tie_c", ["near tie C"], [one(12, "A", 3), one(12, "C", 41), one(12, "A", 20), one(12, "C", 3), one(12, "A", 41),
                                        one(12, "C", 20)], ordered="some")
    add("near_tie_a", ["near tie A"], [one(12, "C", 3), one(12, "A", 41), one(12, "C", 20), one(12, "A", 3), one(12, "C", 41),
                                        one(12, "A", 20)], ordered="some")
    add("clear_winner", ["clear winner"], [one(12, "A", 30, i % 2 == 1) for i in range(10)] + [one(12, "C", 30)], ordered="none")
    add("heads_tails", ["leading S", "trailing S", "ends in I", "starts with D", "one-base read", "refskip spans"],
        [rd(10, "2S5M3S", "TTGCTTATTT", 30), rd(10, "5M2I", "GCTTAGG", 30, True), rd(10, "2D5M", "TTAGG", 30),
         rd(11, "3M4N3M", "CTTCAT", 30), rd(12, "1M", "T", 30, True), rd(14, "1M", "G", 30)])
    # consensus indels: bi / bd are the reads' indel qualities
    add("ins_wins", ["insertion wins"],
        [rd(10, "3M1I3M", "GCTAAGG", 30, bi=30, bd=30), rd(10, "3M1I3M", "GCTAAGG", 30, True, bi=30, bd=10),
         rd(10, "6M", "GCTTAG", 30, bi=40, bd=40)])
    add("idq_decides", ["min_plp_idq decides"],
        [rd(10, "3M1I3M", "GCTAAGG", 30, bi=30, bd=30), rd(10, "3M1I3M", "GCTAAGG", 30, True, bi=30, bd=10),
         rd(10, "6M", "GCTTAG", 30, bi=40, bd=40)], idq=25)
    add("ins_equal", ["event equals non-event"],
        [rd(10, "3M1I3M", "GCTAAGG", 30, bi=20, bd=30), rd(10, "3M1I3M", "GCTAAGG", 30, True, bi=20, bd=30),
         rd(10, "6M", "GCTTAG", 30, bi=40, bd=40)])
    add("two_events_tie", ["two events tie"],
        [rd(10, "3M1I3M", "GCTCAGG", 30, bi=30, bd=30), rd(10, "3M1I3M", "GCTAAGG", 30, True, bi=30, bd=30),
         rd(10, "6M", "GCTTAG", 30, bi=10, bd=40)])
    add("ins_before_del", ["insertion before deletion"],
        [rd(10, "3M2I3M", "GCTGGAGG", 30, bi=30, bd=5), rd(10, "3M2I3M", "GCTGGAGG", 30, True, bi=30, bd=5),
         rd(10, "3M2D3M", "GCTGGC", 30, bi=5, bd=30), rd(10, "3M2D3M", "GCTGGC", 30, True, bi=5, bd=30)])
    add("del_wins", ["deletion wins"],
        [rd(10, "3M2D3M", "GCTGGC", 30, bi=30, bd=30), rd(10, "3M2D3M", "GCTGGC", 30, True, bi=30, bd=30),
         rd(10, "6M", "GCTTAG", 30, bi=40, bd=40)])
    add("region_cut", ["region cut"], [rd(5, "15M", "GCAAGCTTAGGCATC", 30), rd(7, "12M", "AAGCTTAGGCAT", 25, True)],
        begin=9, end=14)
    add("empty_region", ["empty region"], [rd(5, "15M", "GCAAGCTTAGGCATC", 30)], begin=9, end=9)
    add("max_depth_2", ["max_depth drops"], [rd(10, "4M", "GCTT", 30), rd(10, "4M", "GCTA", 30, True), rd(10, "4M", "GCAT", 30),
                                              rd(10, "4M", "CCTT", 30, True), rd(10, "4M", "GGTT", 30)], depth=2)
    return rows


# the header lines, written down (checked against tests/plpsummary_ref.py by test_plpsummary_edges_ref.py)
EXPECT = {
    'window_63': {
        16: 'edge\t17\tC\tT\tA:2/1\tC:2/1\tG:2/1\tT:2/1\tN:0/0\theads:13\ttails:0\tins:0\tdels:0\thrun:1\n',
        17: 'edge\t18\tA\tC\tA:4/1\tC:4/3\tG:4/2\tT:5/2\tN:0/0\theads:13\ttails:0\tins:0\tdels:0\thrun:1\n',
        18: 'edge\t19\tT\tA\tA:7/3\tC:6/3\tG:6/4\tT:6/3\tN:0/0\theads:12\ttails:0\tins:0\tdels:0\thrun:1\n',
        19: 'edge\t20\tC\tC\tA:7/3\tC:9/4\tG:9/4\tT:8/5\tN:0/0\theads:13\ttails:0\tins:0\tdels:0\thrun:1\n',
        20: 'edge\t21\tG\tG\tA:9/6\tC:10/5\tG:11/5\tT:11/5\tN:0/0\theads:12\ttails:13\tins:0\tdels:0\thrun:1\n',
        21: 'edge\t22\tA\tT\tA:9/3\tC:8/4\tG:8/4\tT:9/4\tN:0/0\theads:0\ttails:13\tins:0\tdels:0\thrun:1\n',
        22: 'edge\t23\tT\tC\tA:5/2\tC:7/3\tG:6/3\tT:6/3\tN:0/0\theads:0\ttails:12\tins:0\tdels:0\thrun:1\n',
        23: 'edge\t24\tC\tG\tA:4/2\tC:4/2\tG:5/2\tT:4/2\tN:0/0\theads:0\ttails:13\tins:0\tdels:0\thrun:2\n',
        24: 'edge\t25\tG\tA\tA:2/1\tC:2/1\tG:2/1\tT:2/1\tN:0/0\theads:0\ttails:12\tins:0\tdels:0\thrun:2\n',
    },
    'window_64': {
        16: 'edge\t17\tC\tT\tA:2/1\tC:2/1\tG:2/1\tT:2/1\tN:0/0\theads:13\ttails:0\tins:0\tdels:0\thrun:1\n',
        17: 'edge\t18\tA\tC\tA:4/1\tC:4/3\tG:4/2\tT:5/2\tN:0/0\theads:13\ttails:0\tins:0\tdels:0\thrun:1\n',
        18: 'edge\t19\tT\tG\tA:7/3\tC:6/3\tG:7/4\tT:6/3\tN:0/0\theads:13\ttails:0\tins:0\tdels:0\thrun:1\n',
        19: 'edge\t20\tC\tC\tA:7/3\tC:9/5\tG:8/4\tT:9/5\tN:0/0\theads:13\ttails:0\tins:0\tdels:0\thrun:1\n',
        20: 'edge\t21\tG\tG\tA:10/6\tC:10/5\tG:11/6\tT:10/5\tN:0/0\theads:12\ttails:13\tins:0\tdels:0\thrun:1\n',
        21: 'edge\t22\tA\tT\tA:8/3\tC:9/4\tG:8/4\tT:9/5\tN:0/0\theads:0\ttails:13\tins:0\tdels:0\thrun:1\n',
        22: 'edge\t23\tT\tG\tA:5/3\tC:6/3\tG:7/3\tT:6/3\tN:0/0\theads:0\ttails:13\tins:0\tdels:0\thrun:1\n',
        23: 'edge\t24\tC\tC\tA:4/2\tC:4/3\tG:4/2\tT:4/2\tN:0/0\theads:0\ttails:13\tins:0\tdels:0\thrun:2\n',
        24: 'edge\t25\tG\tA\tA:2/1\tC:2/1\tG:2/1\tT:2/1\tN:0/0\theads:0\ttails:12\tins:0\tdels:0\thrun:2\n',
    },
    'window_65': {
        16: 'edge\t17\tC\tT\tA:2/1\tC:2/1\tG:2/1\tT:2/1\tN:0/0\theads:13\ttails:0\tins:0\tdels:0\thrun:1\n',
        17: 'edge\t18\tA\tC\tA:4/1\tC:4/3\tG:4/2\tT:5/2\tN:0/0\theads:13\ttails:0\tins:0\tdels:0\thrun:1\n',
        18: 'edge\t19\tT\tG\tA:7/3\tC:6/3\tG:7/4\tT:6/3\tN:0/0\theads:13\ttails:0\tins:0\tdels:0\thrun:1\n',
        19: 'edge\t20\tC\tC\tA:7/3\tC:9/5\tG:8/4\tT:9/5\tN:0/0\theads:13\ttails:0\tins:0\tdels:0\thrun:1\n',
        20: 'edge\t21\tG\tA\tA:11/6\tC:10/5\tG:11/6\tT:10/5\tN:0/0\theads:13\ttails:13\tins:0\tdels:0\thrun:1\n',
        21: 'edge\t22\tA\tT\tA:8/3\tC:10/4\tG:8/4\tT:9/5\tN:0/0\theads:0\ttails:13\tins:0\tdels:0\thrun:1\n',
        22: 'edge\t23\tT\tG\tA:5/3\tC:6/3\tG:8/3\tT:6/3\tN:0/0\theads:0\ttails:13\tins:0\tdels:0\thrun:1\n',
        23: 'edge\t24\tC\tC\tA:4/2\tC:4/3\tG:4/2\tT:5/2\tN:0/0\theads:0\ttails:13\tins:0\tdels:0\thrun:2\n',
        24: 'edge\t25\tG\tA\tA:3/1\tC:2/1\tG:2/1\tT:2/1\tN:0/0\theads:0\ttails:13\tins:0\tdels:0\thrun:2\n',
    },
    'window_128': {
        16: 'edge\t17\tC\tT\tA:4/2\tC:4/2\tG:4/2\tT:5/2\tN:0/0\theads:26\ttails:0\tins:0\tdels:0\thrun:1\n',
        17: 'edge\t18\tA\tC\tA:8/3\tC:8/6\tG:9/4\tT:8/4\tN:0/0\theads:26\ttails:0\tins:0\tdels:0\thrun:1\n',
        18: 'edge\t19\tT\tG\tA:12/5\tC:13/6\tG:12/8\tT:13/6\tN:0/0\theads:25\ttails:0\tins:0\tdels:0\thrun:1\n',
        19: 'edge\t20\tC\tT\tA:16/8\tC:17/8\tG:17/9\tT:17/10\tN:0/0\theads:26\ttails:0\tins:0\tdels:0\thrun:1\n',
        20: 'edge\t21\tG\tC\tA:19/10\tC:22/10\tG:21/10\tT:21/11\tN:0/0\theads:25\ttails:26\tins:0\tdels:0\thrun:1\n',
        21: 'edge\t22\tA\tC\tA:14/8\tC:17/9\tG:18/8\tT:17/8\tN:0/0\theads:0\ttails:26\tins:0\tdels:0\thrun:1\n',
        22: 'edge\t23\tT\tC\tA:12/6\tC:12/7\tG:13/6\tT:13/6\tN:0/0\theads:0\ttails:25\tins:0\tdels:0\thrun:1\n',
        23: 'edge\t24\tC\tG\tA:8/4\tC:8/4\tG:8/5\tT:9/4\tN:0/0\theads:0\ttails:26\tins:0\tdels:0\thrun:2\n',
        24: 'edge\t25\tG\tC\tA:3/2\tC:5/2\tG:4/2\tT:4/2\tN:0/0\theads:0\ttails:25\tins:0\tdels:0\thrun:2\n',
    },
    'window_129': {
        16: 'edge\t17\tC\tT\tA:4/2\tC:4/2\tG:4/2\tT:5/2\tN:0/0\theads:26\ttails:0\tins:0\tdels:0\thrun:1\n',
        17: 'edge\t18\tA\tC\tA:8/3\tC:8/6\tG:9/4\tT:8/4\tN:0/0\theads:26\ttails:0\tins:0\tdels:0\thrun:1\n',
        18: 'edge\t19\tT\tG\tA:12/5\tC:13/6\tG:12/8\tT:14/6\tN:0/0\theads:26\ttails:0\tins:0\tdels:0\thrun:1\n',
        19: 'edge\t20\tC\tC\tA:17/8\tC:18/8\tG:17/9\tT:16/10\tN:0/0\theads:26\ttails:0\tins:0\tdels:0\thrun:1\n',
        20: 'edge\t21\tG\tC\tA:19/10\tC:22/10\tG:22/10\tT:21/11\tN:0/0\theads:25\ttails:26\tins:0\tdels:0\thrun:1\n',
        21: 'edge\t22\tA\tC\tA:14/8\tC:17/9\tG:18/8\tT:18/8\tN:0/0\theads:0\ttails:26\tins:0\tdels:0\thrun:1\n',
        22: 'edge\t23\tT\tA\tA:13/6\tC:12/7\tG:13/6\tT:13/6\tN:0/0\theads:0\ttails:26\tins:0\tdels:0\thrun:1\n',
        23: 'edge\t24\tC\tG\tA:7/4\tC:9/4\tG:8/5\tT:9/4\tN:0/0\theads:0\ttails:26\tins:0\tdels:0\thrun:2\n',
        24: 'edge\t25\tG\tA\tA:4/2\tC:4/2\tG:4/2\tT:4/2\tN:0/0\theads:0\ttails:25\tins:0\tdels:0\thrun:2\n',
    },
    'only_d': {
        10: 'edge\t11\tC\tG\tA:0/0\tC:0/0\tG:1/0\tT:0/0\tN:0/0\theads:1\ttails:0\tins:0\tdels:0\thrun:2\n',
        11: 'edge\t12\tT\tC\tA:0/0\tC:1/0\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        12: 'edge\t13\tT\tT\tA:0/0\tC:0/0\tG:0/0\tT:1/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:1\thrun:1\n',
        13: 'edge\t14\tA\tA\tA:0/0\tC:0/0\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        14: 'edge\t15\tG\tA\tA:0/0\tC:0/0\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        15: 'edge\t16\tG\tG\tA:0/0\tC:0/0\tG:1/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:1\n',
        16: 'edge\t17\tC\tG\tA:0/0\tC:0/0\tG:1/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:1\n',
        17: 'edge\t18\tA\tC\tA:0/0\tC:1/0\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:1\tins:0\tdels:0\thrun:1\n',
    },
    'below_bq': {
        12: 'edge\t13\tT\tA\tA:0/0\tC:0/0\tG:0/0\tT:0/0\tN:0/0\theads:3\ttails:3\tins:0\tdels:0\thrun:1\n',
    },
    'q0_dbl_min': {
        12: 'edge\t13\tT\tC\tA:0/0\tC:1/1\tG:0/0\tT:0/0\tN:0/0\theads:2\ttails:2\tins:0\tdels:0\thrun:1\n',
    },
    'cap_93_120': {
        12: 'edge\t13\tT\tA\tA:1/0\tC:0/0\tG:0/0\tT:1/0\tN:0/0\theads:2\ttails:2\tins:0\tdels:0\thrun:1\n',
    },
    'cap_93_94': {
        12: 'edge\t13\tT\tA\tA:0/1\tC:1/0\tG:0/0\tT:0/0\tN:0/0\theads:2\ttails:2\tins:0\tdels:0\thrun:1\n',
    },
    'n_and_iupac': {
        12: 'edge\t13\tT\tT\tA:0/0\tC:0/0\tG:0/0\tT:2/0\tN:1/1\theads:4\ttails:4\tins:0\tdels:0\thrun:1\n',
        13: 'edge\t14\tA\tN\tA:0/0\tC:0/0\tG:0/0\tT:0/0\tN:2/0\theads:2\ttails:2\tins:0\tdels:0\thrun:2\n',
    },
    'exact_tie': {
        12: 'edge\t13\tT\tA\tA:1/1\tC:1/1\tG:0/0\tT:0/0\tN:0/0\theads:4\ttails:4\tins:0\tdels:0\thrun:1\n',
    },
    'near_tie_c': {
        12: 'edge\t13\tT\tC\tA:3/0\tC:3/0\tG:0/0\tT:0/0\tN:0/0\theads:6\ttails:6\tins:0\tdels:0\thrun:1\n',
    },
    'near_tie_a': {
        12: 'edge\t13\tT\tA\tA:3/0\tC:3/0\tG:0/0\tT:0/0\tN:0/0\theads:6\ttails:6\tins:0\tdels:0\thrun:1\n',
    },
    'clear_winner': {
        12: 'edge\t13\tT\tA\tA:5/5\tC:1/0\tG:0/0\tT:0/0\tN:0/0\theads:11\ttails:11\tins:0\tdels:0\thrun:1\n',
    },
    'heads_tails': {
        10: 'edge\t11\tC\tG\tA:0/0\tC:0/0\tG:1/1\tT:0/0\tN:0/0\theads:2\ttails:0\tins:0\tdels:0\thrun:2\n',
        11: 'edge\t12\tT\tC\tA:0/0\tC:2/1\tG:0/0\tT:0/0\tN:0/0\theads:1\ttails:0\tins:0\tdels:0\thrun:2\n',
        12: 'edge\t13\tT\tT\tA:0/0\tC:0/0\tG:0/0\tT:3/2\tN:0/0\theads:1\ttails:1\tins:0\tdels:0\thrun:1\n',
        13: 'edge\t14\tA\tT\tA:0/0\tC:0/0\tG:0/0\tT:3/1\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        14: 'edge\t15\tG\tA\tA:2/1\tC:0/0\tG:1/0\tT:0/0\tN:0/0\theads:1\ttails:3\tins:1\tdels:0\thrun:2\n',
        15: 'edge\t16\tG\tG\tA:0/0\tC:0/0\tG:1/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:1\n',
        16: 'edge\t17\tC\tG\tA:0/0\tC:0/0\tG:1/0\tT:0/0\tN:0/0\theads:0\ttails:1\tins:0\tdels:0\thrun:1\n',
        17: 'edge\t18\tA\tA\tA:0/0\tC:0/0\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:1\n',
        18: 'edge\t19\tT\tC\tA:0/0\tC:1/0\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:1\n',
        19: 'edge\t20\tC\tA\tA:1/0\tC:0/0\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:1\n',
        20: 'edge\t21\tG\tT\tA:0/0\tC:0/0\tG:0/0\tT:1/0\tN:0/0\theads:0\ttails:1\tins:0\tdels:0\thrun:1\n',
    },
    'ins_wins': {
        10: 'edge\t11\tC\tG\tA:0/0\tC:0/0\tG:2/1\tT:0/0\tN:0/0\theads:3\ttails:0\tins:0\tdels:0\thrun:2\n',
        11: 'edge\t12\tT\tC\tA:0/0\tC:2/1\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        12: 'edge\t13\tT\t+A\tA:0/0\tC:0/0\tG:0/0\tT:2/1\tN:0/0\theads:0\ttails:0\tins:2\tdels:0\thrun:1\n',
        13: 'edge\t14\tA\tA\tA:1/1\tC:0/0\tG:0/0\tT:1/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        14: 'edge\t15\tG\tG\tA:1/0\tC:0/0\tG:1/1\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        15: 'edge\t16\tG\tG\tA:0/0\tC:0/0\tG:2/1\tT:0/0\tN:0/0\theads:0\ttails:3\tins:0\tdels:0\thrun:1\n',
    },
    'idq_decides': {
        10: 'edge\t11\tC\tG\tA:0/0\tC:0/0\tG:2/1\tT:0/0\tN:0/0\theads:3\ttails:0\tins:0\tdels:0\thrun:2\n',
        11: 'edge\t12\tT\tC\tA:0/0\tC:2/1\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        12: 'edge\t13\tT\tT\tA:0/0\tC:0/0\tG:0/0\tT:2/1\tN:0/0\theads:0\ttails:0\tins:1\tdels:0\thrun:1\n',
        13: 'edge\t14\tA\tA\tA:1/1\tC:0/0\tG:0/0\tT:1/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        14: 'edge\t15\tG\tG\tA:1/0\tC:0/0\tG:1/1\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        15: 'edge\t16\tG\tG\tA:0/0\tC:0/0\tG:2/1\tT:0/0\tN:0/0\theads:0\ttails:3\tins:0\tdels:0\thrun:1\n',
    },
    'ins_equal': {
        10: 'edge\t11\tC\tG\tA:0/0\tC:0/0\tG:2/1\tT:0/0\tN:0/0\theads:3\ttails:0\tins:0\tdels:0\thrun:2\n',
        11: 'edge\t12\tT\tC\tA:0/0\tC:2/1\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        12: 'edge\t13\tT\tT\tA:0/0\tC:0/0\tG:0/0\tT:2/1\tN:0/0\theads:0\ttails:0\tins:2\tdels:0\thrun:1\n',
        13: 'edge\t14\tA\tA\tA:1/1\tC:0/0\tG:0/0\tT:1/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        14: 'edge\t15\tG\tG\tA:1/0\tC:0/0\tG:1/1\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        15: 'edge\t16\tG\tG\tA:0/0\tC:0/0\tG:2/1\tT:0/0\tN:0/0\theads:0\ttails:3\tins:0\tdels:0\thrun:1\n',
    },
    'two_events_tie': {
        10: 'edge\t11\tC\tG\tA:0/0\tC:0/0\tG:2/1\tT:0/0\tN:0/0\theads:3\ttails:0\tins:0\tdels:0\thrun:2\n',
        11: 'edge\t12\tT\tC\tA:0/0\tC:2/1\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        12: 'edge\t13\tT\t+C\tA:0/0\tC:0/0\tG:0/0\tT:2/1\tN:0/0\theads:0\ttails:0\tins:2\tdels:0\thrun:1\n',
        13: 'edge\t14\tA\tA\tA:1/1\tC:0/0\tG:0/0\tT:1/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        14: 'edge\t15\tG\tG\tA:1/0\tC:0/0\tG:1/1\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        15: 'edge\t16\tG\tG\tA:0/0\tC:0/0\tG:2/1\tT:0/0\tN:0/0\theads:0\ttails:3\tins:0\tdels:0\thrun:1\n',
    },
    'ins_before_del': {
        10: 'edge\t11\tC\tG\tA:0/0\tC:0/0\tG:2/2\tT:0/0\tN:0/0\theads:4\ttails:0\tins:0\tdels:0\thrun:2\n',
        11: 'edge\t12\tT\tC\tA:0/0\tC:2/2\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        12: 'edge\t13\tT\t+GG\tA:0/0\tC:0/0\tG:0/0\tT:2/2\tN:0/0\theads:0\ttails:0\tins:2\tdels:2\thrun:1\n',
        13: 'edge\t14\tA\tA\tA:1/1\tC:0/0\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        14: 'edge\t15\tG\tG\tA:0/0\tC:0/0\tG:1/1\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        15: 'edge\t16\tG\tG\tA:0/0\tC:0/0\tG:2/2\tT:0/0\tN:0/0\theads:0\ttails:2\tins:0\tdels:0\thrun:1\n',
        16: 'edge\t17\tC\tG\tA:0/0\tC:0/0\tG:1/1\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:1\n',
        17: 'edge\t18\tA\tC\tA:0/0\tC:1/1\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:2\tins:0\tdels:0\thrun:1\n',
    },
    'del_wins': {
        10: 'edge\t11\tC\tG\tA:0/0\tC:0/0\tG:2/1\tT:0/0\tN:0/0\theads:3\ttails:0\tins:0\tdels:0\thrun:2\n',
        11: 'edge\t12\tT\tC\tA:0/0\tC:2/1\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        12: 'edge\t13\tT\t-AG\tA:0/0\tC:0/0\tG:0/0\tT:2/1\tN:0/0\theads:0\ttails:0\tins:0\tdels:2\thrun:1\n',
        13: 'edge\t14\tA\tT\tA:0/0\tC:0/0\tG:0/0\tT:1/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        14: 'edge\t15\tG\tA\tA:1/0\tC:0/0\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        15: 'edge\t16\tG\tG\tA:0/0\tC:0/0\tG:2/1\tT:0/0\tN:0/0\theads:0\ttails:1\tins:0\tdels:0\thrun:1\n',
        16: 'edge\t17\tC\tG\tA:0/0\tC:0/0\tG:1/1\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:1\n',
        17: 'edge\t18\tA\tC\tA:0/0\tC:1/1\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:2\tins:0\tdels:0\thrun:1\n',
    },
    'region_cut': {
        9: 'edge\t10\tG\tG\tA:0/0\tC:0/0\tG:1/1\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:1\n',
        10: 'edge\t11\tC\tC\tA:0/0\tC:1/1\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        11: 'edge\t12\tT\tT\tA:0/0\tC:0/0\tG:0/0\tT:1/1\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        12: 'edge\t13\tT\tT\tA:0/0\tC:0/0\tG:0/0\tT:1/1\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:1\n',
        13: 'edge\t14\tA\tA\tA:1/1\tC:0/0\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
    },
    'empty_region': {
    },
    'max_depth_2': {
        10: 'edge\t11\tC\tG\tA:0/0\tC:0/0\tG:1/1\tT:0/0\tN:0/0\theads:2\ttails:0\tins:0\tdels:0\thrun:2\n',
        11: 'edge\t12\tT\tC\tA:0/0\tC:1/1\tG:0/0\tT:0/0\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:2\n',
        12: 'edge\t13\tT\tT\tA:0/0\tC:0/0\tG:0/0\tT:1/1\tN:0/0\theads:0\ttails:0\tins:0\tdels:0\thrun:1\n',
        13: 'edge\t14\tA\tA\tA:0/1\tC:0/0\tG:0/0\tT:1/0\tN:0/0\theads:0\ttails:2\tins:0\tdels:0\thrun:2\n',
    },
}
