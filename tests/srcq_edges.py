"""Reads at the routing boundaries of the source-quality kernel (lofreq_amd/csrc/lfq_srcq.hip): K = non-matches - 1 on either
side of LFQ_SRCQ_LDS_CELLS (the DP cells in LDS or in the wavefront's scratch slice), on either side of the 64 and 128 cells the
lanes stride over, and the two ends of the pruning exit, which is part of the result.

Every read is built so that count_cigar_ops (samutils.c:437-614) counts exactly m non-matches among n operations; count()
below recounts them the way it does, and the table asserts K = m - 1.  Two regimes per K:
  all     n = m: every counted operation is a non-match, the exit `n > K` cannot fire before the last row (ops_all_a, ops_all_b)
  early   non-matches among twice as many matches, half of them of quality 0: the tail passes 0.05 early (ops_early)
The reference is oracle.source_qual (held to the SQ track of the 2.1.4 binary by tests/test_source_qual.py)."""
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")
MIN_BQ = 0                      # every base is counted: a quality of 0 is an error probability of 1
INDEL_QUAL = 45


def source_constants():
    def find(fname, pattern):
        m = re.search(pattern, open(os.path.join(CSRC, fname)).read(), re.M)
        assert m, "%s: nothing matches %r" % (fname, pattern)
        return int(m.group(1))
    c = {"LDS_CELLS": find("lfq_internal.h", r"^#define\s+LFQ_SRCQ_LDS_CELLS\s+(\d+)\b"),
         "WAVES": find("lfq_srcq.hip", r"^#define\s+LFQ_SRCQ_WAVES\s+(\d+)\b"),
         "STRIDE": find("lfq_srcq.hip", r"for \(int k = lane; k <= top; k \+= (\d+)\)"),
         "BLOCKS_PER_CU": find("lfq_readset.hip", r"std::min<int64_t>\(\(n \+ 3\) / 4, \(int64_t\)c->n_cu \* (\d+)\)\);")}
    assert re.search(r"if \(K < LFQ_SRCQ_LDS_CELLS\) \{", open(os.path.join(CSRC, "lfq_srcq.hip")).read())
    assert re.search(r"if \(n > K && prev\[K\] > 0\.05\) \{", open(os.path.join(CSRC, "lfq_srcq.hip")).read())
    assert find("lfq_srcq.hip", r"^#define\s+LFQ_SRCQ_INDEL_QUAL\s+(\d+)\b") == INDEL_QUAL
    return c


C = source_constants()
LDS_CELLS, WAVES, STRIDE = C["LDS_CELLS"], C["WAVES"], C["STRIDE"]
K_SET = (1, 2, STRIDE - 2, STRIDE - 1, STRIDE, STRIDE + 1, 2 * STRIDE - 1, 2 * STRIDE, 2 * STRIDE + 1,
         LDS_CELLS - 2, LDS_CELLS - 1, LDS_CELLS, LDS_CELLS + 1)

REF_LEN = 6000
_rng = np.random.default_rng(9901)
GENOME = _rng.integers(0, 4, REF_LEN).astype(np.uint8)
REF = bytes(b"ACGT"[c] for c in GENOME)


def make_read(name, ops, pos0, seed=0, indels=False):
    """a read whose counted operations are `ops`, [(non-match, quality)], in seeded order over M and X operations: a match
    copies the contig, a non-match does not; indels: an insertion and a deletion on top (two more non-matches of quality 45)"""
    rng = np.random.default_rng([seed, len(ops), pos0])
    ops = [ops[i] for i in rng.permutation(len(ops))]
    block = [o for o in ops if o[0]][:len(ops) // 4]            # an X operation in the middle: non-matches only
    rest = list(ops)
    for o in block:
        rest.remove(o)
    cut = len(rest) // 2
    cigar, seq, qual, x = [], [], [], pos0
    for i, (op, part) in enumerate((("M", rest[:cut]), ("X", block), ("M", rest[cut:]))):
        for wrong, q in part:
            b = int(GENOME[x])
            seq.append((b + 1 + int(rng.integers(3))) % 4 if wrong else b)
            qual.append(q)
            x += 1
        if part:
            cigar.append((op, len(part)))
        if indels and i == 0:
            cigar.append(("I", 2))
            seq.extend(int(v) for v in rng.integers(0, 4, 2))
            qual.extend([30, 30])
        if indels and i == 1:
            cigar.append(("D", 3))
            x += 3
    assert x <= REF_LEN, name
    return {"name": name, "pos0": int(pos0), "cigar": cigar, "seq": np.asarray(seq, np.uint8), "qual": np.asarray(qual, np.uint8),
            "K": sum(1 for w, _ in ops if w) + (2 if indels else 0) - 1}


# The result is (int)(-10 log10(1 - P(X = K - 1))): it says something only where that probability is large, so the qualities are
# chosen to put it there -- non-matches of quality 0 (error probability 1) carry the mass one cell a row through all K cells,
# a few of quality 1 .. 3 and 20 spread it.
def ops_all_a(K):
    """n = m = K + 1: one non-match of quality 3, K of quality 0.  After K rows the tail is 0.5 already, but n > K is not true
    before the last row, which takes cell K - 1 from 0.5 to 0"""
    return [(True, 3)] + [(True, 0)] * K


def ops_all_b(K):
    """n = m = K + 1: two non-matches of quality 20, one of quality 1, the others of quality 0: cell K - 1 ends near 0.78"""
    q = [20, 1, 20]
    return [(True, v) for v in (q[:K + 1] if K + 1 <= len(q) else q + [0] * (K + 1 - len(q)))]


def ops_early(K):
    """n = 3 K + 11: one non-match of quality 10, K of quality 0, among K + 10 matches of quality 41 and K of quality 0.  The
    rows of quality 0 move the mass up a cell each; the tail reaches 0.1 more than K rows before the last one, with 0.9 in
    cell K - 1, which the next row would empty"""
    return [(True, 10)] + [(True, 0)] * K + [(False, 41)] * (K + 10) + [(False, 0)] * K


def count(r, min_bq=MIN_BQ):
    """(counted operations n, counted non-matches m) of one read, the way count_cigar_ops counts them"""
    n = m = 0
    x, y = r["pos0"], 0
    for op, l in r["cigar"]:
        if op in "MX":
            for j in range(l):
                if r["qual"][y + j] < min_bq:
                    continue
                n += 1
                m += 1 if op == "X" or (x + j >= REF_LEN or GENOME[x + j] != r["seq"][y + j]) else 0
            x, y = x + l, y + l
        elif op in "ID":
            n, m = n + 1, m + 1
            x, y = (x, y + l) if op == "I" else (x + l, y)
        elif op == "N":
            x += l
        elif op == "S":
            y += l
    return n, m


def exit_row(r, min_bq=MIN_BQ):
    """(the row at which the kernel's loop leaves, the number of rows n) in plain doubles: the recurrence of lfq_srcq_dp
    restated, rows in ascending error probability"""
    n_ops, m = count(r, min_bq)
    K = m - 1
    quals, y = [], 0
    for op, l in r["cigar"]:
        if op in "MX":
            quals += [int(v) for v in r["qual"][y:y + l] if v >= min_bq]
        elif op in "ID":
            quals.append(INDEL_QUAL)
        y += l if op in "MXIS" else 0
    prev = np.zeros(K + 1)
    prev[0] = 1.0
    for n, q in enumerate(sorted(quals, reverse=True), 1):
        p = 10.0 ** (-q / 10.0)
        cur = prev * (1.0 - p)
        cur[1:] += prev[:-1] * p
        cur[K] = prev[K] + prev[K - 1] * p
        prev = cur
        if n > K and prev[K] > 0.05:
            return n, n_ops
    return n_ops, n_ops


Row = namedtuple("Row", "name kind reads")
N_MANY = 2600           # more reads than a launch has wavefronts (4 per block, two blocks per compute unit, 256 of those)


def boundary_table():
    t = []
    for K in K_SET:
        t.append(Row("K %d" % K, "K", [make_read("K%d_all_a" % K, ops_all_a(K), 10 + K % 7, seed=1),
                                       make_read("K%d_all_b" % K, ops_all_b(K), 20 + K % 5, seed=2),
                                       make_read("K%d_early" % K, ops_early(K), 30 + K % 3, seed=3)]))
    a, b = LDS_CELLS - 1, LDS_CELLS
    t.append(Row("LDS and scratch in neighbouring wavefronts: K %d between two K %d" % (b, a), "neighbours",
                 [make_read("n0_K%d" % a, ops_all_b(a), 5, seed=11), make_read("n1_K%d" % b, ops_all_b(b), 6, seed=12),
                  make_read("n2_K%d" % a, ops_early(a), 7, seed=13), make_read("n3_K%d" % b, ops_early(b), 8, seed=14),
                  make_read("n4_K%d" % a, ops_all_a(a), 9, seed=15), make_read("n5_K%d" % b, ops_all_a(b), 10, seed=16)]))
    many = []
    ks = (1, 2, 5, STRIDE - 1, STRIDE, STRIDE + 1, 9, 3)
    rng = np.random.default_rng(31)
    for i in range(N_MANY):
        K = ks[i % len(ks)]
        kind = (i // len(ks)) % 4
        if kind == 3:               # seeded qualities, with an insertion and a deletion
            ops = [(True, int(v)) for v in rng.choice([0, 0, 0, 1, 2, 3, 20], K - 1)] + [(False, int(v)) for v in rng.choice([0, 3, 30, 41], 12)]
        else:
            ops = (ops_all_a, ops_all_b, ops_early)[kind](K)
        many.append(make_read("g%d_K%d" % (i, K), ops, (i * 2) % (REF_LEN - 400), seed=100 + i, indels=kind == 3 and K >= 2))
    t.append(Row("more reads than the launch has wavefronts", "grid", many))
    return t


def row_id(row):
    return re.sub(r"[^A-Za-z0-9]+", "_", row.name.split(":")[0]).strip("_")
