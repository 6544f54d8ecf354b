"""Plain-Python restatement of the header line of `lofreq plpsummary` (plp_summary, lofreq_call.c:445-459) from reads: what
compile_plp_col (plp.c:797-1288) leaves in fw_counts / rv_counts, num_heads, num_tails, num_ins, num_dels, hrun and cons_base.
Test infrastructure, no device, numpy only for the reads' arrays.

Reads are the dicts of lofreq_amd.ReadSet: pos0, cigar [(op, len)], seq (codes 0..4 = ACGTN, 5..15 any other IUPAC code),
qual (phred), mapq, reverse, and optionally bi / bd (tag bytes, quality + 33).  They are in file (= pileup) order.

The walk is mpileup's: one cursor per read (resolve_cigar2 of htslib), advanced position by position; the entries of a
position are visited in read order, and base_counts is a sequential double sum in that order, with math.pow -- the libm
pow() of the reference's `1.0 - PHREDQUAL_TO_PROB(bq)` (utils.h:42)."""
import math
import sys

NT4 = "ACGTN"                   # bam_nt4_rev_table
SEQ_LETTERS = "ACGTN=MRSVWYHKDB"   # the read set's base codes (lofreq_amd.encode_seq): 0..4 as NT4, 5..15 the other BAM letters
SANGER_PHRED_MAX = 93           # defaults.h:32
DBL_MIN = sys.float_info.min


def argmax_d(vals):
    """utils.c:87-98: the FIRST maximum"""
    best = 0
    for i in range(1, len(vals)):
        if vals[i] > vals[best]:
            best = i
    return best


def get_hrun(pos, ref):
    """plp.c:744-787: the homopolymer run an indel after `pos` would sit in"""
    n = len(ref)
    hrun = 1
    if pos + 1 >= n:
        return hrun
    c = ref[pos + 1].upper()
    i = pos + 2
    while i < n and ref[i].upper() == c:
        hrun += 1
        i += 1
    i = pos
    while i >= 0 and ref[i].upper() == c:
        hrun += 1
        i -= 1
    return hrun


class Cursor:
    """one read's position in its CIGAR (bam_plp's resolve_cigar2): entry(p) for p = pos0, pos0 + 1, ... -> None past the end,
    else (is_del, qpos, indel, is_head, is_tail)"""

    def __init__(self, read):
        self.cig = [(op, l) for op, l in read["cigar"]]
        self.pos0 = read["pos0"]
        self.l_qseq = len(read["seq"])
        self.end = self.pos0 + sum(l for op, l in self.cig if op in "MDN=X")      # bam_endpos
        self.k, self.x, self.y = 0, self.pos0, 0         # operation, its first reference position, its first query position

    def _peek(self, k):
        """the indel that follows operation k: +len for I, -len for D; a P in between: the inserted bases behind it"""
        if k + 1 >= len(self.cig):
            return 0
        op2, l2 = self.cig[k + 1]
        if op2 == "D":
            return -l2
        if op2 == "I":
            return l2
        if op2 == "P" and k + 2 < len(self.cig):
            l3 = 0
            for op3, n3 in self.cig[k + 2:]:
                if op3 == "I":
                    l3 += n3
                elif op3 in "DMN=X":
                    break
            return l3 if l3 > 0 else 0
        return 0

    def entry(self, p):
        if p < self.pos0 or p >= self.end:
            return None
        while True:                                   # advance to the reference-consuming operation that holds p
            op, l = self.cig[self.k]
            if op in "M=X" or op in "DN":
                if p < self.x + l:
                    break
                self.x += l
                if op in "M=X":
                    self.y += l
            elif op in "IS":
                self.y += l
            self.k += 1
        is_del = op in "DN"
        qpos = self.y if is_del else self.y + (p - self.x)
        qpos = min(qpos, self.l_qseq - 1)
        indel = self._peek(self.k) if p == self.x + l - 1 else 0
        return is_del, qpos, indel, p == self.pos0, p == self.end - 1


def summarize(reads, ref, begin, end, min_plp_bq=3, min_plp_idq=0, keep=None):
    """-> list of column dicts (covered positions of [begin, end), in order): pos0, ref, cons, fw[5], rv[5], heads, tails, ins,
    dels, hrun, coverage.  keep: the mask of a -d cap (tests/maxdepth_model.py), None = every read"""
    reads = [r for i, r in enumerate(reads) if keep is None or keep[i]]
    cursors = [Cursor(r) for r in reads]
    cols = []
    first = 0                                          # reads before `first` end before the current position
    for p in range(begin, end):
        base_counts = [0.0] * 5                        # plp.c:808
        fw, rv = [0] * 5, [0] * 5
        heads = tails = n_ins = n_dels = cov = 0
        nonevent = [0, 0]                              # ins_nonevent_qual, del_nonevent_qual (:810)
        events = [{}, {}]                              # key -> cons_quals; dicts keep insertion order as uthash does
        while first < len(reads) and cursors[first].end <= p:
            first += 1
        for r, c in zip(reads[first:], cursors[first:]):
            if r["pos0"] > p:
                break
            e = c.entry(p)
            if e is None:
                continue
            is_del, qpos, indel, is_head, is_tail = e
            cov += 1
            if not is_del:                             # :912
                heads += 1 if is_head else 0
                tails += 1 if is_tail else 0
                code = int(r["seq"][qpos])
                nt4 = code if code < 4 else 4          # seq_nt16_int
                bq = int(r["qual"][qpos])
                if bq >= min_plp_bq:                   # :937
                    if bq > SANGER_PHRED_MAX:          # :949-953
                        bq = SANGER_PHRED_MAX
                    incr = 1.0 - math.pow(10.0, -1.0 * bq / 10.0)      # :999
                    if incr == 0.0:                    # :1003-1005
                        incr = DBL_MIN
                    base_counts[nt4] += incr
                    if r["reverse"]:
                        rv[nt4] += 1
                    else:
                        fw[nt4] += 1
            iq = int(r["bi"][qpos]) - 33 if r.get("bi") is not None else 0       # :1024-1059
            dq = int(r["bd"][qpos]) - 33 if r.get("bd") is not None else 0
            if iq < min_plp_idq or dq < min_plp_idq:   # :1062
                continue
            if indel > 0:                              # :1072-1112
                n_ins += 1
                key = "".join(SEQ_LETTERS[int(r["seq"][qpos + j])] if qpos + j < len(r["seq"]) else "N"
                              for j in range(1, indel + 1))              # seq_nt16_str of the inserted bases, upper case
                events[0][key] = events[0].get(key, 0) + iq
                nonevent[1] += dq
            elif indel < 0:                            # :1116-1168
                n_dels += 1
                key = "".join(ref[p + j].upper() if p + j < len(ref) else "N" for j in range(1, -indel + 1))
                events[1][key] = events[1].get(key, 0) + dq
                nonevent[0] += iq
            else:                                      # :1170-1191
                nonevent[0] += iq
                nonevent[1] += dq
        if cov == 0:
            continue
        best = []
        for sd in range(2):                            # :1231-1248: the first event whose sum is strictly greatest
            bk, bq_ = None, 0
            for key, q in events[sd].items():
                if q > bq_:
                    bk, bq_ = key, q
            best.append((bk, bq_))
        if not best[0][1] > nonevent[0] and not best[1][1] > nonevent[1]:       # :1255-1268
            cons = NT4[argmax_d(base_counts)]
        elif best[0][1] > nonevent[0]:
            cons = "+" + best[0][0]
        else:
            cons = "-" + best[1][0]
        rb = ref[p] if p < len(ref) else "N"           # :818-823
        if rb not in "ACTGN":
            rb = "N"
        cols.append({"pos0": p, "ref": rb, "cons": cons, "fw": fw, "rv": rv, "heads": heads, "tails": tails, "ins": n_ins,
                     "dels": n_dels, "hrun": get_hrun(p, ref), "coverage": cov, "base_counts": base_counts})
    return cols


def format_line(chrom, c):
    """lofreq_call.c:445-459"""
    s = "%s\t%d\t%s\t%s" % (chrom, c["pos0"] + 1, c["ref"], c["cons"])
    for i in range(5):
        s += "\t%s:%d/%d" % (NT4[i], c["fw"][i], c["rv"][i])
    s += "\theads:%d\ttails:%d" % (c["heads"], c["tails"])
    s += "\tins:%d\tdels:%d" % (c["ins"], c["dels"])
    s += "\thrun:%d" % c["hrun"]
    return s + "\n"


def lines(chrom, reads, ref, begin, end, **kw):
    return [format_line(chrom, c) for c in summarize(reads, ref, begin, end, **kw)]


def load_golden(name):
    """tests/golden/<name>.json (tests/make_plpsummary_golden.py) -> (fixture, reads as dicts)"""
    import json
    import os

    import numpy as np
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".json")))
    code = {c: i for i, c in enumerate(SEQ_LETTERS)}
    tag = lambda t: None if t is None else np.frombuffer(t.encode(), np.uint8)
    reads = [{"pos0": r[0], "cigar": _parse_cigar(r[3]), "seq": np.array([code.get(c, 4) for c in r[4].upper()], np.uint8),
              "qual": np.array([ord(c) - 33 for c in r[5]], np.uint8), "mapq": r[2], "reverse": bool(r[1] & 16),
              "bi": tag(r[6]), "bd": tag(r[7])} for r in fx["reads"]]
    return fx, reads


def _parse_cigar(s):
    import re
    return [(op, int(n)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", s)]
