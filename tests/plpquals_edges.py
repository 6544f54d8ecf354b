"""Tiny inputs on the constants of lfq_plp_group_kernel (lfq_pileup.hip) and on the branches of plp_summary's quality lines
(lofreq_call.c:460-598).

Used by test_plpquals_edges_ref.py (CPU: the rows sit where their names say, every branch of BRANCHES has a row) and by
test_gpu_plpquals.py (the kernel, the host layer and the formatters against the same rows).  Every expected value comes from the
restatement tests/plpquals_ref.py, which test_plpquals_ref.py holds to the reference's binary.

Two kinds of rows:
  TrackRow  host SNV tracks (numpy; nt bits 0-2 code, bit 3 strand), a column range and a flag.  expect = (nt_off, bq, baq, mq,
            sq) of plpquals_ref.group_tracks and `text`, the nucleotide lines of every column of the range.
  ReadRow   reads for lofreq_amd.ReadSet (dicts, pileup order), region and options.  expect = the complete text of
            `lofreq plpsummary`, one string per covered position (plpquals_ref.text).
"""
import os
import re
from collections import namedtuple

import numpy as np

import maxdepth_model as mdm
import plpquals_ref as Q
from plpsummary_edges import CHROM, REF, one, rd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TrackRow = namedtuple("TrackRow", "name branches nt bq baq mq sq col_off c0 c1 flag expect text")
ReadRow = namedtuple("ReadRow", "name branches reads ref begin end min_plp_bq min_plp_idq max_depth flag expect")

BRANCHES = (
    "depth 0", "depth 1", "depth 63", "depth 64", "depth 65", "depth 128", "depth 129",
    "five groups, no lane keeps its place", "one group", "only N", "IUPAC code",
    "ncols 1", "ncols 4", "ncols 5", "range starts off a word", "no baq track", "sq 254 and 255", "baq 255", "mq 255",
    "all below min_plp_bq", "max_depth drops", "two insertions and a deletion", "events on one side", "no event",
)


def kernel_constants():
    """(observations a round, columns a workgroup) of lfq_plp_group_kernel, read from the source"""
    src = open(os.path.join(ROOT, "lofreq_amd", "csrc", "lfq_pileup.hip")).read()
    body = src[src.index("void lfq_plp_group_kernel("):]
    body = body[:body.index("int lfq_launch_plp_group(")]
    rounds = {int(x) for x in re.findall(r"r0 \+= (\d+)\)", body)}
    cols = {int(x) for x in re.findall(r"blockIdx\.x \* (\d+)", body)}
    assert len(rounds) == 1 and len(cols) == 1
    return rounds.pop(), cols.pop()


def _tracks(depths, code, seed, baq=True, sq=False):
    """columns of the given depths; code(c, i) -> the nt code of observation i of column c; the quality bytes are seeded and all
    different enough that a misplaced observation shows"""
    rng = np.random.default_rng(seed)
    n = int(sum(depths))
    col_off = np.zeros(len(depths) + 1, np.uint64)
    col_off[1:] = np.cumsum(depths)
    nt = np.zeros(n, np.uint8)
    k = 0
    for c, d in enumerate(depths):
        for i in range(d):
            nt[k] = code(c, i) | (8 if (i * 5 + c) % 3 == 0 else 0)
            k += 1
    bq = rng.integers(3, 42, n).astype(np.uint8)
    mq = rng.choice(np.array([0, 20, 37, 60, 255], np.uint8), n)
    b = rng.integers(0, 70, n).astype(np.uint8) if baq else None
    s = rng.integers(0, 60, n).astype(np.uint8) if sq else None
    return nt, bq, b, mq, s, col_off


def table():
    W, G = kernel_constants()
    rows = []

    def tracks(name, branches, t, c0=0, c1=None, flag=Q.LFQ_USE_BAQ):
        nt, bq, baq, mq, sq, col_off = t
        c1 = len(col_off) - 1 if c1 is None else c1
        if baq is None:
            flag &= ~Q.LFQ_USE_BAQ
        exp = Q.group_tracks(nt, bq, baq, mq, sq, col_off, c0, c1)
        text = [Q.format_grouped(*exp, i, flag) for i in range(c1 - c0)]
        rows.append(TrackRow(name, tuple(branches), nt, bq, baq, mq, sq, col_off, c0, c1, flag, exp, text))

    def reads(name, branches, rds, begin=0, end=len(REF), bq=3, idq=0, depth=None, flag=Q.LFQ_USE_BAQ):
        keep = mdm.kept_reads(rds, depth) if depth is not None else None
        exp = Q.text(CHROM, rds, REF, begin, end, flag, bq, idq, keep)
        rows.append(ReadRow(name, tuple(branches), rds, REF, begin, end, bq, idq, depth, flag, exp))

    mixed = lambda c, i: (i * 3 + c) % 5
    for d in (1, W - 1, W, W + 1, 2 * W, 2 * W + 1):
        # the column under test between two short neighbours: a store past either end lands in their bytes
        tracks("depth_%d" % d, ["depth %d" % d], _tracks([3, d, 2], mixed, 100 + d))
    tracks("depth_0", ["depth 0"], _tracks([5, 0, 0, 4, 0], mixed, 7))
    tracks("five_groups", ["five groups, no lane keeps its place"], _tracks([W + 1], lambda c, i: (i + 2) % 5, 8))
    tracks("one_group", ["one group"], _tracks([W + 6], lambda c, i: 2, 9))
    tracks("only_n", ["only N"], _tracks([9], lambda c, i: 4, 10))
    tracks("iupac", ["IUPAC code"], _tracks([11], lambda c, i: (0, 5, 4, 6, 1, 7)[i % 6], 11))
    for n in (1, G, G + 1):
        tracks("ncols_%d" % n, ["ncols %d" % n], _tracks([2 + (3 * c) % 7 for c in range(n)], mixed, 20 + n))
    tracks("range_offset_3", ["range starts off a word"], _tracks([3, 6, 2, 7, 5], mixed, 30), c0=1, c1=4)
    tracks("no_baq", ["no baq track"], _tracks([6, 7], mixed, 31, baq=False))
    t = _tracks([8, 70], mixed, 32, sq=True)
    t[4][[0, 3, 9, 77]] = 254
    t[4][[1, 10, 76]] = 255
    t[2][[2, 11, 70]] = 255
    t[3][[4, 12]] = 255
    tracks("sq_baq_mq_missing", ["sq 254 and 255", "baq 255", "mq 255"], t, flag=Q.LFQ_USE_BAQ | Q.LFQ_USE_SQ)

    reads("below_bq", ["all below min_plp_bq"], [one(12, "T", 2), one(12, "G", 1, True), one(12, "T", 0)])
    reads("max_depth_2", ["max_depth drops"],
          [one(12, "A", 30), one(12, "C", 31, True), one(12, "G", 32), one(12, "T", 33), one(12, "A", 34, mapq=20)], depth=2)
    two_one = [rd(10, "3M1I3M", "GCTAAGG", 30, bi=30, bd=31), rd(10, "3M2I3M", "GCTCCAGG", 31, True, bi=32, bd=33, mapq=20),
               rd(10, "3M1I3M", "GCTAAGG", 32, bi=34, bd=35, mapq=0), rd(10, "3M2D3M", "GCTGCA", 33, True, bi=36, bd=37),
               rd(10, "6M", "GCRTAG", 34, bi=38, bd=39, mapq=255), rd(11, "5M", "CTNAG", 35, True, bi=40, bd=41)]
    reads("two_ins_one_del", ["two insertions and a deletion", "no event", "IUPAC code"], two_one)
    reads("one_side", ["events on one side"],
          [rd(10, "3M2D3M", "GCTGCA", 30, bi=30, bd=31), rd(10, "3M2D3M", "GCTGCA", 31, True, bi=32, bd=33),
           rd(10, "8M", "GCTTAGGC", 32, bi=34, bd=35)], begin=11, end=14)
    # the same reads with lb / ai / ad tags: BAQ and AQ values other than -1
    tagged = []
    for i, r in enumerate(two_one):
        r = dict(r)
        n = len(r["seq"])
        r["lb"] = np.array([33 + (i * 7 + j * 3) % 60 for j in range(n)], np.uint8)
        r["ai"] = np.array([33 + (i * 5 + j) % 50 for j in range(n)], np.uint8)
        r["ad"] = np.array([33 + (i * 3 + j * 2) % 50 for j in range(n)], np.uint8)
        tagged.append(r)
    reads("tagged", ["two insertions and a deletion"], tagged)
    return rows
