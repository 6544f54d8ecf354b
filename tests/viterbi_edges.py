"""Reads at the geometry boundaries of the viterbi kernels (lofreq_amd/csrc/lfq_viterbi.hip): 64 query rows a strip, one
anti-diagonal a step, four steps a dword of back pointers, a hand-over row loaded 64 columns at a time, the window clipped at
both contig ends, the first-maximum tie rule, the quality median of the gather kernel.

  geometry        the window rule of vit_scan restated (lower = max(pos - RWIN, 0), upper = min(x + RWIN, ref_len)) and what
                  the kernel makes of it: q, w, n_strips, rows of the last strip, its n_steps; and whether the read is one the
                  2.1.4 binary can be asked about (in_binary_domain, below)
  mk              a read that follows a contig along its CIGAR
  boundary_table  named rows of one or a few reads; a read carries the geometry its row's name claims ("claim"), written
                  down here, not computed
  main            writes tests/golden/viterbi_edges.json: the model's result of every read and -q value, and the binary's for
                  the reads in its domain (tests/make_viterbi_golden.py: run_binary)

The binary is no reference for every read the library takes: fetch_func holds the window in
char ref[l_qseq + 1 + indels + 2 * RWIN] (lofreq_viterbi.c:251) and the alignment in malloc(2 * l_qseq) (:262), and writes past
either without looking.  A read is in its domain only when w <= l_qseq + n_indel_ops + 2 * RWIN and the alignment is shorter
than 2 * l_qseq.  By that rule one deletion of d >= 2 bases is d - 1 bytes outside already: the rows that ask for a 2-base
deletion have a twin with a 1-base deletion (or a 2-base insertion), which is inside.

    python tests/viterbi_edges.py          (LFQ_GOLDEN_OUT: another output directory)
"""
import json
import os
import re
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import viterbi_model as vm  # noqa: E402

SRC = os.path.join(ROOT, "lofreq_amd", "csrc", "lfq_viterbi.hip")
FIXTURE = os.path.join(HERE, "golden", "viterbi_edges.json")
DEF_QUALS = (-1, 0, 20, 93)         # every -q the fixture holds; a row runs with (-1, 20) unless it says otherwise


# ---- the constants, read from the source ------------------------------------------------------------------------------

def source_constants():
    text = open(SRC).read()

    def find(pattern):
        m = re.search(pattern, text)
        assert m, "lfq_viterbi.hip: nothing matches %r" % pattern
        return [int(v) for v in m.groups()]
    c = {}
    c["RWIN"], = find(r"#define\s+LFQ_VIT_RWIN\s+(\d+)\b")
    add, shift = find(r"const int n_strips = \(q \+ (\d+)\) >> (\d+);")
    c["STRIP"] = 1 << shift
    assert add == c["STRIP"] - 1
    assert find(r"const int rows = min\((\d+), q - \(s << (\d+)\)\);") == [c["STRIP"], shift]
    assert find(r"const int i = \(s << (\d+)\) \+ lane \+ 1;") == [shift]
    load, = find(r"for \(int tb = 0; tb < n_steps; tb \+= (\d+)\)")
    c["LOAD"] = load                                                    # columns of the hand-over row per load
    inner, pack = find(r"for \(int tt = 0; tt < (\d+) && tb \+ tt < n_steps; tt \+= (\d+)\)")
    assert inner == load
    c["PACK"] = pack                                                    # steps per dword of back pointers
    assert find(r"return \(int64_t\)\(\(w \+ 63 \+ 3\) / (\d+)\) \* (\d+);") == [pack, 4 * c["STRIP"]]
    c["GATHER"], = find(r"for \(int64_t b = lane; b < len && z \+ b < R\.base_off \+ R\.q; b \+= (\d+)\)")
    assert re.search(r"if \(s > 0 && kk <= w\) \{", text) and re.search(r"const double v_start = i == 1 \? 0\.0 : IMIN;", text)
    return c


C = source_constants()
RWIN, STRIP, PACK, LOAD, GATHER = C["RWIN"], C["STRIP"], C["PACK"], C["LOAD"], C["GATHER"]
assert RWIN == vm.RWIN


# ---- the contigs ------------------------------------------------------------------------------------------------------

PA_AT, PA_LEN = 1000, 220               # A x 220
AT_AT, AT_UNITS = 1500, 40              # (AT) x 40
LOW_AT, LOW_LEN = 2000, 40              # lower case
MAIN_LEN, SHORT_LEN = 3000, 90


def make_contigs():
    rng = np.random.default_rng(8801)
    g = list(rng.choice(list("ACGT"), MAIN_LEN))
    g[PA_AT:PA_AT + PA_LEN] = "A" * PA_LEN
    g[PA_AT - 1], g[PA_AT + PA_LEN] = "C", "G"
    g[AT_AT:AT_AT + 2 * AT_UNITS] = "AT" * AT_UNITS
    g[AT_AT - 1], g[AT_AT + 2 * AT_UNITS] = "G", "C"
    g[LOW_AT:LOW_AT + LOW_LEN] = [c.lower() for c in g[LOW_AT:LOW_AT + LOW_LEN]]
    return {"main": "".join(g), "short": "".join(rng.choice(list("ACGT"), SHORT_LEN))}


CONTIGS = make_contigs()


# ---- reads and their geometry -----------------------------------------------------------------------------------------

def mk(name, contig, pos0, cigar, qual=None, ins=None, seed=0, claim=None):
    """a read of CONTIGS[contig] that follows it from pos0 along `cigar` (a string); inserted and clipped bases are seeded
    unless `ins` gives the bases of every I in order; qual: None (seeded, 8 .. 41), a number, or a list"""
    G = CONTIGS[contig].upper()
    cigar = vm.parse_cigar(cigar)
    rng = np.random.default_rng([seed, pos0] + [l for _, l in cigar])
    ins = list(ins or [])
    seq, x = [], pos0
    for op, l in cigar:
        if op in "M=X":
            assert x + l <= len(G), name
            seq.extend(G[x:x + l])
            x += l
        elif op == "I" and ins:
            s = ins.pop(0)
            assert len(s) == l
            seq.extend(s)
        elif op in "IS":
            seq.extend(rng.choice(list("ACGT"), l))
        elif op == "D":
            x += l
    if qual is None:
        qual = [int(v) for v in rng.integers(8, 42, len(seq))]
    elif np.isscalar(qual):
        qual = [int(qual)] * len(seq)
    assert len(qual) == len(seq), name
    return {"name": name, "contig": contig, "pos0": int(pos0), "cigar": cigar, "seq": "".join(seq), "qual": [int(v) for v in qual],
            "claim": dict(claim or {})}


Geom = namedtuple("Geom", "q w n_strips rows n_steps lower upper l_qseq n_indel_ops")


def geometry(r):
    """vit_scan's window of one read and the kernel's strips over it"""
    ref_len = len(CONTIGS[r["contig"]])
    x, z, indels = r["pos0"], 0, 0
    for op, l in r["cigar"]:
        if op in "M=X":
            x, z = x + l, z + l
        elif op == "I":
            z, indels = z + l, indels + 1
        elif op == "D":
            x, indels = x + l, indels + 1
    lower = max(r["pos0"] - RWIN, 0)
    upper = min(x + RWIN, ref_len)
    q, w = z, upper - lower
    n_strips = (q + STRIP - 1) // STRIP
    rows = q - (n_strips - 1) * STRIP
    return Geom(q, w, n_strips, rows, w + rows - 1, lower, upper, len(r["seq"]), indels)


def lib_read(r):
    return {"pos0": r["pos0"], "cigar": r["cigar"], "seq": np.asarray([vm.LETTERS.index(c) for c in r["seq"]], np.uint8),
            "qual": np.asarray(r["qual"], np.uint8)}


_MODEL = {}


def model_result(r, dq):
    """[pos0, cigar string, status] of tests/viterbi_model.py; -q matters to a read with a quality of 2 only"""
    key = (r["contig"], r["pos0"], vm.cigar_str(r["cigar"]), r["seq"], bytes(r["qual"]), dq if 2 in r["qual"] else None)
    if key not in _MODEL:
        p, c, s = vm.realign(lib_read(r), CONTIGS[r["contig"]], dq)
        _MODEL[key] = [p, vm.cigar_str(c), s]
    return list(_MODEL[key])


def in_binary_domain(r, model):
    """the window fits ref[] and the alignment fits aln[] (with its terminator) in fetch_func; model: model_result(r, dq)"""
    g = geometry(r)
    aln = sum(l for op, l in vm.parse_cigar(model[1]) if op in "MID")
    return g.w <= g.l_qseq + g.n_indel_ops + 2 * RWIN and aln < 2 * g.l_qseq


# ---- the table --------------------------------------------------------------------------------------------------------

Row = namedtuple("Row", "name kind contig reads dqs")
KINDS = ("pad", "q", "w", "n_steps", "w<q", "w>>q", "strip edge", "clipped", "tie", "quality", "gather")
Q_SET = (2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321)
W_SET = (63, 64, 65, 127, 128, 129, 191, 192, 193)
EDGE_ROWS = (63, 64, 65, 127, 128)
LONG_DELS = (100, 300, 400, 600)
ORD = 1650                              # ordinary sequence behind the repeats (the lower-case stretch lies inside it)
ORD0 = 100                              # ... and in front of them


def boundary_table():
    t = []

    def add(name, kind, reads, contig="main", dqs=(-1, 20)):
        assert kind in KINDS and len({r["name"] for r in reads}) == len(reads) and all(r["contig"] == contig for r in reads), name
        assert set(dqs) <= set(DEF_QUALS)
        t.append(Row(name, kind, contig, reads, tuple(dqs)))

    # ---- the four plain realigned reads a row is put behind
    add("pad main", "pad", [mk("pad%d" % i, "main", 300 + 11 * i, "30M1D30M", seed=900 + i) for i in range(4)])
    add("pad short", "pad", [mk("spad%d" % i, "short", 12 + 3 * i, "20M1D20M", seed=910 + i) for i in range(4)], contig="short")
    # ---- query length: rows 1 .. 64 of the last strip, 1 to 17 strips
    add("q 1: 1I and 1M2D", "q", [mk("q1_1I", "main", ORD0, "1I", claim=dict(q=1, n_strips=1, rows=1, w=2 * RWIN)),
                                  mk("q1_1M2D", "main", ORD0 + 40, "1M2D", claim=dict(q=1, n_strips=1, rows=1, w=3 + 2 * RWIN)),
                                  mk("q1_1M1D", "main", ORD0 + 80, "1M1D", claim=dict(q=1, w=2 + 2 * RWIN))])
    for q in Q_SET:
        a = q // 2
        claim = dict(q=q, n_strips=(q + 63) // 64, rows=(q - 1) % 64 + 1)
        add("q %d: a 2-base deletion in the middle, and its 1-base twin" % q, "q",
            [mk("q%d_2D" % q, "main", ORD, "%dM2D%dM" % (a, q - a), seed=q, claim=dict(claim, w=q + 2 + 2 * RWIN)),
             mk("q%d_1D" % q, "main", ORD + 7, "%dM1D%dM" % (a, q - a), seed=q + 1, claim=dict(claim, w=q + 1 + 2 * RWIN))])
    add("q 1030: 17 strips", "q", [mk("q1030_2D", "main", ORD, "500M2D530M", seed=5, claim=dict(q=1030, n_strips=17, rows=6)),
                                   mk("q1030_1D", "main", ORD + 3, "500M1D530M", seed=6, claim=dict(q=1030, n_strips=17, rows=6))])
    # ---- window length: the kk <= w guard of the hand-over load and the w + 1 stride of its rows (two strips each)
    for w in W_SET:
        q = w - 1 - 2 * RWIN
        reads = [mk("w%d" % w, "main", ORD0 + 20, "%dM1D%dM" % (q // 2, q - q // 2), seed=w, claim=dict(w=w, q=q))]
        q2 = w + 40                     # the same window under a read of two or more strips: a 60-base insertion
        reads.append(mk("w%d_strips" % w, "main", ORD0 + 400, "%dM60I%dM" % ((q2 - 60) // 2, q2 - 60 - (q2 - 60) // 2), seed=w + 1,
                        claim=dict(w=w, q=q2, n_strips=(q2 + 63) // 64)))
        add("w %d" % w, "w", reads)
    # ---- steps of the last strip: every residue modulo the pack of four, and 0, 1, 63 modulo the 64 columns of a load
    steps = []
    for q, cg, n in ((22, "11M1D11M", 64), (23, "11M1D12M", 66), (24, "11M2I11M", 65), (23, "10M2I11M", 63),
                     (86, "43M1D43M", 128), (88, "43M2I43M", 129), (87, "42M2I43M", 127), (87, "43M1D44M", 130)):
        steps.append(mk("steps%d_q%d" % (n, q), "main", ORD0 + 10 * len(steps), cg, seed=n, claim=dict(q=q, n_steps=n)))
    add("n_steps of the last strip 63 .. 66 and 127 .. 130", "n_steps", steps)
    # ---- the last column of the hand-over row (kk == w): a trailing insertion behind the contig's last base puts the rows of the
    # next strips into V_I of column w, whose row above is the hand-over row's last entry
    add("w: a trailing insertion behind the contig end, in column w across rows 64 and 128", "w",
        [mk("tail_ins64", "main", MAIN_LEN - 50, "50M30I", seed=1, claim=dict(w=50 + RWIN, q=80, n_strips=2)),
         mk("tail_ins128", "main", MAIN_LEN - 100, "100M40I", seed=2, claim=dict(w=100 + RWIN, q=140, n_strips=3))])
    # ---- the window shorter than the query
    add("w < q: 10M100I10M", "w<q", [mk("ins100", "main", ORD0, "10M100I10M", seed=1, claim=dict(q=120, w=40, n_strips=2))])
    add("w < q: more than 128 query bases over fewer than 64 columns", "w<q",
        [mk("ins110", "main", ORD0 + 50, "15M110I15M", seed=2, claim=dict(q=140, w=50, n_strips=3))])
    # ---- the window much longer than the query: the optimum is a long insertion, the trace-back walks I across strips
    for d in LONG_DELS:
        add("w >> q: 40M%dD40M" % d, "w>>q", [mk("del%d" % d, "main", ORD, "40M%dD40M" % d, seed=d, claim=dict(q=80, w=80 + d + 2 * RWIN))])
    add("w >> q: 50M600D50M, two strips", "w>>q", [mk("del600_q100", "main", ORD + 5, "50M600D50M", seed=9,
                                                      claim=dict(q=100, n_strips=2, w=700 + 2 * RWIN))])
    # ---- an indel on a strip edge
    for r in EDGE_ROWS:
        add("strip edge: an insertion and a deletion directly after row %d" % r, "strip edge",
            [mk("edge%d_3I" % r, "main", ORD, "%dM3I40M" % r, seed=r), mk("edge%d_1D" % r, "main", ORD + 9, "%dM1D40M" % r, seed=r + 1),
             mk("edge%d_5D" % r, "main", ORD + 18, "%dM5D40M" % r, seed=r + 2)])
    add("strip edge: an insertion of 3 bases on rows 63 to 65", "strip edge", [mk("edge_span", "main", ORD + 30, "62M3I40M", seed=3)])
    # ---- the window clipped by a contig end
    clip = [mk("pos%d" % p, "main", p, "30M1D30M", seed=p, claim=dict(w=min(p, RWIN) + 61 + RWIN)) for p in (0, 3, 9, 10, 11)]
    add("clipped: pos 0, 3, 9, 10, 11", "clipped", clip)
    add("clipped: the read ends at ref_len, ref_len - 9, ref_len - 10", "clipped",
        [mk("end%d" % e, "main", MAIN_LEN - 61 - e, "30M1D30M", seed=20 + e, claim=dict(w=RWIN + 61 + min(e, RWIN))) for e in (0, 9, 10)])
    add("clipped: at both ends of the 90-base contig", "clipped",
        [mk("both4", "short", 4, "40M1D40M", seed=1, claim=dict(w=SHORT_LEN, q=80)),
         mk("both0", "short", 0, "44M1D45M", seed=2, claim=dict(w=SHORT_LEN, q=89)),
         mk("both_ins", "short", 2, "40M3I40M", seed=3, claim=dict(w=SHORT_LEN, q=83))], contig="short")
    # ---- ties: every start column of a one-letter window scores bit-identically, every unit of a repeat likewise
    pa = PA_AT + 60
    for label, qual in (("quality 30", 30), ("quality 2 but one base", [2] * 17 + [30] + [2] * 42)):
        qi = qual if np.isscalar(qual) else qual + [2]
        add("tie: poly-A, a deletion and an insertion inside, %s" % label, "tie",
            [mk("pa_del", "main", pa, "30M1D30M", qual=qual), mk("pa_ins", "main", pa + 5, "30M1I30M", qual=qi, ins=["A"]),
             mk("pa_del2", "main", pa + 9, "30M2D30M", qual=qual)])
    # the last base, a C of quality 93, is better inserted than mismatched: V_I of the last row is the same double in every
    # column the whole read fits in front of, and the strict > of the termination keeps the first one
    add("tie: poly-A, the last base inserted, V_I of the last row equal in every column", "tie",
        [mk("pa_last_ins", "main", pa, "30M1I", qual=[30] * 30 + [93], ins=["C"]),
         mk("pa_last_ins_strips", "main", pa + 3, "70M1I", qual=[30] * 70 + [93], ins=["C"])])
    span = 2 * AT_UNITS + 40            # 20 bases of ordinary sequence on either side of the repeat
    at = []
    for where, a in (("left", 20), ("middle", 20 + AT_UNITS), ("right", 20 + 2 * AT_UNITS - 2)):
        at.append(mk("at_del_%s" % where, "main", AT_AT - 20, "%dM2D%dM" % (a, span - 2 - a), qual=30))
        at.append(mk("at_ins_%s" % where, "main", AT_AT - 20, "%dM2I%dM" % (a, span - a), qual=30, ins=["AT"]))
    add("tie: one unit of the (AT) repeat deleted / inserted at its left, middle and right, quality 30", "tie", at)
    # ---- qualities
    q2run = [30] * 80
    q2run[10:25] = [2] * 15
    q2run[70:] = [2] * 10
    one = [2] * 80
    one[33] = 17
    even = [2] * 76 + [10, 20, 31, 40]  # four qualities other than 2: the median pair 20, 31 has an odd sum
    ends = [30] * 80
    ends[0], ends[41], ends[79] = 0, 93, 0
    add("quality: runs of Q2, one quality other than 2, an even count with an odd median sum, 0 and 93", "quality",
        [mk("q2_runs", "main", ORD0, "40M1D40M", qual=q2run, seed=1), mk("q2_but_one", "main", ORD0 + 5, "40M1D40M", qual=one, seed=2),
         mk("q2_even_median", "main", ORD0 + 9, "40M2I38M", qual=even, seed=3), mk("q0_q93", "main", ORD0 + 14, "40M1D40M", qual=ends, seed=4),
         mk("q93_all", "main", ORD0 + 20, "20M1D20M", qual=93, seed=5), mk("q0_all", "main", ORD0 + 25, "20M1D20M", qual=0, seed=6)],
        dqs=DEF_QUALS)
    # ---- the gather kernel of the resident path: operations longer than its lane stride and twice that
    rq = np.random.default_rng(77)
    g1 = [int(v) for v in rq.integers(2, 42, 70 + 100 + 70 + 30)]
    g2 = [int(v) for v in rq.integers(2, 42, 130 + 140 + 130 + 20 + 70)]
    add("gather: M, I and S longer than 64 and than 128, a leading S directly in front of an I", "gather",
        [mk("ops70", "main", ORD, "70S100M70I30M", qual=g1, seed=1), mk("ops130", "main", ORD + 4, "130S140M130I20M70S", qual=g2, seed=2),
         mk("s_then_i", "main", ORD + 8, "5S3I60M", seed=3), mk("m200_1D", "main", ORD + 12, "200M1D3M", seed=4)])
    assert len({row_id(r) for r in t}) == len(t)
    return t


def row_id(row):
    return re.sub(r"[^A-Za-z0-9]+", "_", row.name.replace("<", "lt").replace(">>", "gg")).strip("_")


def pad_reads(table, contig):
    """the four plain realigned reads of `contig` that a row's reads are put behind"""
    (row,) = [r for r in table if r.kind == "pad" and r.contig == contig]
    return row.reads


# ---- the fixture ------------------------------------------------------------------------------------------------------

def load_fixture():
    return json.load(open(FIXTURE))


def inline_read(r):
    return [r["name"], r["pos0"], vm.cigar_str(r["cigar"]), r["seq"], "".join(chr(33 + v) for v in r["qual"])]


def main():
    import make_viterbi_golden as mg
    table = boundary_table()
    fix = {"name": "viterbi_edges", "generator": "tests/viterbi_edges.py", "reference_binary": "lofreq 2.1.4 (dist tgz)",
           "command": "lofreq viterbi -f t.fa [-q Q] -o out.bam t.sam", "def_quals": list(DEF_QUALS), "contigs": CONTIGS, "rows": []}
    # one run of the binary per contig, over the reads that are in its domain with every -q value
    asked = {c: [] for c in CONTIGS}
    for row in table:
        for r in row.reads:
            if all(in_binary_domain(r, model_result(r, dq)) for dq in DEF_QUALS):
                asked[row.contig].append(dict(r, name=row_id(row) + "." + r["name"]))
            else:
                assert not any(in_binary_domain(r, model_result(r, dq)) for dq in DEF_QUALS), r["name"]
    binary = {}
    mg.DEF_QUALS = list(DEF_QUALS)
    for c, reads in asked.items():
        _, res = mg.run_binary(CONTIGS[c], reads)
        for i, r in enumerate(reads):
            binary[r["name"]] = {str(dq): res[str(dq)][i] for dq in DEF_QUALS}
    for row in table:
        out = {"name": row.name, "contig": row.contig, "def_quals": list(row.dqs), "reads": [inline_read(r) for r in row.reads],
               "model": {}, "binary": {}}
        for dq in row.dqs:
            out["model"][str(dq)] = [model_result(r, dq) for r in row.reads]
            out["binary"][str(dq)] = [binary.get(row_id(row) + "." + r["name"], {}).get(str(dq)) for r in row.reads]
        fix["rows"].append(out)
    mg.dump("viterbi_edges", fix)


if __name__ == "__main__":
    main()
