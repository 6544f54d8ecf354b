"""Reads at the routing and geometry boundaries of the BAQ / IDAQ kernels (lfq_baq.hip, the geometry loop of lfq_readset.hip).

Three pieces, used by test_baq_edges.py (CPU: the table sits where it says, the oracle can be trusted there) and
test_gpu_baq_edges.py (the kernels against the oracle, row by row):

  geometry        the host's geometry of one read restated line by line from lfq_readset.hip (window, band, row width, the
                  kernel the read goes to) plus the per-read fh / bh of lfq_baq_reg_kernel and the wave-wide interior range;
  make_read       a read that follows the contig along its CIGAR, with seeded mismatches, qualities and inserted bases;
  boundary_table  every boundary as a Row: the constant and source line it belongs to, the reads, the route each read must
                  take -- written down here, not computed -- and, for the wavefront rows, the interior range f_hi.

The constants and the cited lines are read from the sources, not restated.
"""
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")
OPS = "MIDNSHP=X"
LETTERS = "ACGTN"


# ---- the constants and the lines, read from the sources --------------------------------------------------------------

def _find(fname, pattern):
    """(match, 'file:line') of the first line of lofreq_amd/csrc/<fname> that holds `pattern` (a regular expression)"""
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
    """{name: (value, 'file:line')} of everything the routing and the kernels' row ranges hang on"""
    c = {}
    for name in ("LFQ_BAQ_LDS_CELLS", "LFQ_BAQ_BAND8_CELLS", "LFQ_BAQ_LDS_MAX_LREF", "LFQ_BAQ_MAX_INDELS", "LFQ_BAQ_MAX_TERMS"):
        c[name] = _define("lfq_internal.h", name)
    c["LFQ_BAQ_NB"] = _define("lfq_baq.hip", "LFQ_BAQ_NB")
    c["LFQ_BAQ_NB_WIDE"] = _define("lfq_baq.hip", "LFQ_BAQ_NB_WIDE")
    lit = re.escape
    m, at = _find("lfq_readset.hip", r"int bw = (\d+);")
    c["default band"] = (int(m.group(1)), at)
    m, at = _find("lfq_readset.hip", lit("if (abs((xe - xb) - (ye - yb)) > bw) bw = abs((xe - xb) - (ye - yb)) + ") + r"(\d+);")
    c["band switch"] = (int(m.group(1)), at)
    c["xb clamp"] = (None, _find("lfq_readset.hip", lit("xb -= yb + bw / 2; if (xb < 0) xb = 0;"))[1])
    c["window trim"] = (None, _find("lfq_readset.hip", lit("xb += (xe - xb - l_qseq - bw) / 2, xe -= (xe - xb - l_qseq - bw) / 2;"))[1])
    c["xe clamp"] = (None, _find("lfq_readset.hip", lit("if (xe > rd->ref_len) xe = (int)rd->ref_len;"))[1])
    c["b2"] = (None, _find("lfq_readset.hip", lit("if (b2 < abs(o.l_ref - l_qseq)) b2 = abs(o.l_ref - l_qseq);"))[1])
    c["row width"] = (None, _find("lfq_readset.hip", lit("wr = (b2 * 2 + 1) * 3 + 6;"))[1])
    c["narrow route"] = (None, _find("lfq_readset.hip", lit("if (use_lds && wr <= LFQ_BAQ_LDS_CELLS && o.l_ref <= LFQ_BAQ_LDS_MAX_LREF) {"))[1])
    c["band8 route"] = (None, _find("lfq_readset.hip", lit("} else if (use_lds && wr == LFQ_BAQ_BAND8_CELLS && o.l_ref <= LFQ_BAQ_LDS_MAX_LREF) {"))[1])
    c["fh"] = (None, _find("lfq_baq.hip", lit("int fh = act ? (bw == BWF ? (l_query < l_ref - BWF ? l_query : l_ref - BWF) : 0) : 1 << 30;"))[1])
    c["bh"] = (None, _find("lfq_baq.hip", lit("int bh = act ? (bw == BWF ? (l_query - 1 < l_ref - BWF - 1 ? l_query - 1 : l_ref - BWF - 1) : 0) : 1 << 30;"))[1])
    c["f_hi"] = (None, _find("lfq_baq.hip", lit("f_hi = fh < BWF + 1 ? 0 : fh;"))[1])
    c["Lmax"] = (None, _find("lfq_baq.hip", lit("int Lmax = l_query;"))[1])
    c["batch clamp"] = (None, _find("lfq_baq.hip", lit("LFQ_BAQ_BATCH((Lmax >> 2) - 1, rB0, rB1, rB2, rB3, eB0, eB1, eB2, eB3);"))[1])
    c["stored rows"] = (None, _find("lfq_baq.hip", lit("const bool store = (i & 1) == 0;"))[1])
    m, at = _find("lfq_baq.hip", r"if \(oplen > (\d+)\) continue;")
    c["oplen skip"] = (int(m.group(1)), at)
    c["qpos 0"] = (None, _find("lfq_baq.hip", lit("if (qpos == 0) continue;"))[1])
    c["table cap"] = (None, _find("lfq_baq.hip", lit("if (n_tab < LFQ_BAQ_MAX_INDELS && n_terms + nt <= LFQ_BAQ_MAX_TERMS) {"))[1])
    c["nt clamp ins"] = (None, _find("lfq_baq.hip", lit("if (qpos + nt > l_query) nt = l_query - qpos;"))[1])
    c["nt clamp del"] = (None, _find("lfq_baq.hip", lit("if (qpos + nt - 1 > l_query) nt = l_query - qpos + 1;"))[1])
    c["repeat scan"] = (None, _find("lfq_baq.hip", lit("while (ref_i < xe) {"))[1])
    c["match ops"] = (None, _find("lfq_readset.hip", lit("if (op == 0 || op == 7 || op == 8) {"))[1])
    c["nflag"] = (None, _find("lfq_baq.hip", lit("if (A.nflag && (A.nflag[blockIdx.x] != 0) != HN) {"))[1])
    c["quality table"] = (None, _find("lfq_baq.hip", lit("s_q2p[t * 64 + lane] = (double)A.qual2prob[t * 64 + lane];"))[1])
    c["qk cap"] = (None, _find("lfq_baq_sweep_row.inc", lit("qk = qk > 100 ? 99 : qk;"))[1])
    return c


C = source_constants()
LDS_CELLS, BAND8_CELLS, MAX_LREF = C["LFQ_BAQ_LDS_CELLS"][0], C["LFQ_BAQ_BAND8_CELLS"][0], C["LFQ_BAQ_LDS_MAX_LREF"][0]
MAX_INDELS, MAX_TERMS = C["LFQ_BAQ_MAX_INDELS"][0], C["LFQ_BAQ_MAX_TERMS"][0]
BW0, BW_ADD, OPLEN_MAX = C["default band"][0], C["band switch"][0], C["oplen skip"][0]
BWF = {"narrow": (C["LFQ_BAQ_NB"][0] - 1) // 2, "band8": (C["LFQ_BAQ_NB_WIDE"][0] - 1) // 2}


# ---- the host geometry of one read (lfq_readset.hip, the loop of lfq_readset_baq) ------------------------------------

Geom = namedtuple("Geom", "bw xb l_ref b2 wr route fh bh")


def geometry(pos0, cigar, l_qseq, ref_len):
    """bw, xb, l_ref as the host computes them; b2 = the band the kernels run with (kprobaln_ext.c:99-101), wr the row
    width, route the kernel; fh / bh = the read's own interior limits in the register kernel (None on the wide route,
    1 << 30 for a lane without a read)"""
    x, y, yb, ye, xb, xe = pos0, 0, -1, -1, -1, -1
    for op, l in cigar:                             # C["match ops"]
        if op in "M=X":
            if yb < 0:
                yb = y
            if xb < 0:
                xb = x
            ye, xe = y + l, x + l
            x += l
            y += l
        elif op in "SI":
            y += l
        elif op in "DN":
            x += l
    bw = BW0
    if abs((xe - xb) - (ye - yb)) > bw:             # C["band switch"]
        bw = abs((xe - xb) - (ye - yb)) + BW_ADD
    xb -= yb + bw // 2                              # C["xb clamp"]
    if xb < 0:
        xb = 0
    xe += l_qseq - ye + bw // 2
    if xe - xb - l_qseq > bw:                       # C["window trim"]: the second half sees the first one's xb
        xb += (xe - xb - l_qseq - bw) // 2
        xe -= (xe - xb - l_qseq - bw) // 2
    if xe > ref_len:                                # C["xe clamp"]
        xe = ref_len
    l_ref = xe - xb
    b2, wr = None, 0
    if l_qseq > 0 and l_ref > 0:
        b2 = min(max(l_ref, l_qseq), bw)
        b2 = max(b2, abs(l_ref - l_qseq))           # C["b2"]
        wr = (b2 * 2 + 1) * 3 + 6                   # C["row width"]
    if wr <= LDS_CELLS and l_ref <= MAX_LREF:       # C["narrow route"]
        route = "narrow"
    elif wr == BAND8_CELLS and l_ref <= MAX_LREF:   # C["band8 route"]
        route = "band8"
    else:
        route = "wide"
    fh = bh = None
    if route != "wide":
        f = BWF[route]
        if b2 is None:
            fh = bh = 1 << 30
        elif b2 == f:                               # C["fh"], C["bh"]
            fh, bh = min(l_qseq, l_ref - f), min(l_qseq - 1, l_ref - f - 1)
        else:
            fh = bh = 0
    return Geom(bw, xb, l_ref, b2, wr, route, fh, bh)


def read_geometry(r, ref_len):
    return geometry(r["pos0"], r["cigar"], len(r["seq"]), ref_len)


def has_indel(r):
    return any(op in "ID" for op, _ in r["cigar"])


def wavefronts(reads, ref_len, idaq=False):
    """the register kernel's wavefronts of one call: [(route, [read index] * <= 64)] in launch order -- the narrow reads in
    input order (with idaq: those without an I / D operation first), then the band-8 reads; the wide reads run in the
    all-HBM kernel, which has no wave-wide state"""
    g = [read_geometry(r, ref_len) for r in reads]
    nar = [i for i in range(len(reads)) if g[i].route == "narrow"]
    if idaq:
        groups = [("narrow", [i for i in nar if not has_indel(reads[i])]), ("narrow", [i for i in nar if has_indel(reads[i])])]
    else:
        groups = [("narrow", nar)]
    groups.append(("band8", [i for i in range(len(reads)) if g[i].route == "band8"]))
    out = []
    for route, idx in groups:
        for a in range(0, len(idx), 64):
            out.append((route, idx[a:a + 64]))
    return out


def wave_state(reads, idx, route, ref_len):
    """(Lmax, f_hi, b_hi) of the wavefront that holds reads[idx] (C["Lmax"], C["f_hi"])"""
    g = [read_geometry(reads[i], ref_len) for i in idx]
    f = BWF[route]
    fh, bh = min(x.fh for x in g), min(x.bh for x in g)
    return max(len(reads[i]["seq"]) for i in idx), (0 if fh < f + 1 else fh), (0 if bh < f + 1 else bh)


def idaq_table(r, ref, ref_len):
    """the indel table of one read as both kernels build it (C["table cap"]): [(kind, qpos, nt, tracked)] of every indel
    the reference gives a quality ('I' / 'D'; qpos = the 1-based base that carries the byte), in CIGAR order"""
    g = read_geometry(r, ref_len)
    xe, l_query = g.xb + g.l_ref, len(r["seq"])
    x, y, n_tab, n_terms, out = r["pos0"], 0, 0, 0, []
    for op, l in r["cigar"]:
        if op in "M=X":
            x += l
            y += l
        elif op == "D":
            rpos, qpos = x, y
            if qpos == 0 or l > OPLEN_MAX:          # C["qpos 0"], C["oplen skip"]: neither advances x
                continue
            x += l
            ref_i, rep, rep_i = x, 0, 0
            while ref_i < xe and ref[ref_i] == ref[rpos + rep_i]:
                rep, ref_i, rep_i = rep + 1, ref_i + 1, (rep_i + 1) % l
            nt = rep + 1
            if qpos + nt - 1 > l_query:             # C["nt clamp del"]
                nt = l_query - qpos + 1
            ok = n_tab < MAX_INDELS and n_terms + nt <= MAX_TERMS
            out.append(("D", qpos, nt, ok))
            if ok:
                n_tab, n_terms = n_tab + 1, n_terms + nt
        elif op == "I":
            qpos = y
            if l > OPLEN_MAX or qpos == 0:          # neither advances y
                continue
            y += l
            ref_i, rep, rep_i = x, 0, 0
            while ref_i < xe and ref[ref_i] == ord(LETTERS[min(int(r["seq"][qpos + rep_i]), 4)]):
                rep, ref_i, rep_i = rep + 1, ref_i + 1, (rep_i + 1) % l
            nt = rep + 1
            if qpos + nt > l_query:                 # C["nt clamp ins"]
                nt = l_query - qpos
            nt = max(nt, 0)
            ok = n_tab < MAX_INDELS and n_terms + nt <= MAX_TERMS
            out.append(("I", qpos, nt, ok))
            if ok:
                n_tab, n_terms = n_tab + 1, n_terms + nt
        elif op == "S":
            y += l
    return out


# ---- the contig and the read builder ---------------------------------------------------------------------------------

HOMO_AT, HOMO_LEN = 1000, 420          # A x 420
AT_AT, AT_LEN = 620, 12                # ATATATATATAT
N_AT = 700
LOWER_AT, LOWER_LEN = 760, 40
REF_LEN = 2000


def make_contig():
    rng = np.random.default_rng(7001)
    g = list(rng.choice(list("ACGT"), REF_LEN))
    g[AT_AT:AT_AT + AT_LEN] = list("AT" * (AT_LEN // 2))
    g[N_AT] = "N"
    g[LOWER_AT:LOWER_AT + LOWER_LEN] = [c.lower() for c in g[LOWER_AT:LOWER_AT + LOWER_LEN]]
    g[HOMO_AT:HOMO_AT + HOMO_LEN] = "A" * HOMO_LEN
    g[HOMO_AT - 1], g[HOMO_AT + HOMO_LEN] = "C", "G"
    return "".join(g).encode()


CONTIG = make_contig()


def make_read(name, pos0, cigar, seed=0, mm=0.02, qual=None, ins=None, ref=CONTIG):
    """A read that follows `ref` from pos0 along `cigar` ([(op, len)]; a string like "10S40M2D50M" works too).  M bases
    mismatch at rate `mm` (seeded), = never, X always; an N of the contig is read as a seeded base; S and I bases are seeded
    unless `ins` gives the inserted bases of every I, in order.  qual: None (seeded, 2 .. 41), an int, or an array."""
    if isinstance(cigar, str):
        cigar = [(op, int(n)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    rng = np.random.default_rng([seed, pos0, len(cigar)] + [l for _, l in cigar])
    ins = list(ins or [])
    seq, x = [], pos0
    for op, l in cigar:
        if op in "M=X":
            for k in range(l):
                c = chr(ref[x + k]).upper()
                other = [b for b in "ACGT" if b != c]
                if c not in "ACGT":
                    c = str(rng.choice(list("ACGT")))
                elif op == "X" or (op == "M" and rng.random() < mm):
                    c = str(rng.choice(other))
                seq.append(c)
            x += l
        elif op == "I" and ins:
            s = ins.pop(0)
            assert len(s) == l
            seq.extend(s)
        elif op in "SI":
            seq.extend(rng.choice(list("ACGT"), l))
        elif op in "DN":
            x += l
    assert x <= len(ref), (name, x)
    n = len(seq)
    if qual is None:
        q = np.clip(np.round(rng.normal(30, 8, n)), 2, 41).astype(np.uint8)
    elif np.isscalar(qual):
        q = np.full(n, qual, np.uint8)
    else:
        q = np.asarray(qual, np.uint8)
        assert len(q) == n
    return {"name": name, "pos0": int(pos0), "cigar": [(op, int(l)) for op, l in cigar],
            "seq": np.array([LETTERS.index(c) for c in seq], np.uint8), "qual": q}


def plain(name, pos0, l, **kw):
    return make_read(name, pos0, [("M", l)], **kw)


def pad_reads():
    """64 plain 100-base reads (one wavefront of the register kernel): what a row's reads are appended to"""
    return [plain("pad%d" % i, 200 + 3 * i, 100, seed=900 + i) for i in range(64)]


# ---- the boundary table ---------------------------------------------------------------------------------------------

# routes: one name for all the reads of the row, or one per read; f_hi: the interior range of the row's first register
# wavefront when its reads run alone without idaq (None: the row does not pin it); overflow: the row runs past an indel
# table cap
Row = namedtuple("Row", "name kind const at reads routes f_hi overflow")

LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65)
MID = 1500                      # ordinary sequence, far from both ends
KINDS = ("length", "interior", "bw<7", "l_ref", "wr", "clips", "idaq", "quality")


def _wave(name, lens, at=MID, seed=0):
    return [plain("%s.%d" % (name, i), at + (i % 40), l, seed=seed + i) for i, l in enumerate(lens)]


def _swap(reads, lane, r):
    out = list(reads)
    out[lane] = r
    return out


def _indel_chain(name, pos0, n_pairs, extra=None, lead=4, seed=0, ins_base=None, ref=CONTIG):
    """2-base matches with 1-base I and D in turn between them: 2 n_pairs indels, net difference 0; `extra` appends one
    more operation pair"""
    cg = [("M", lead)]
    n_ins = 0
    for _ in range(n_pairs):
        cg += [("I", 1), ("M", 2), ("D", 1), ("M", 2)]
        n_ins += 1
    if extra:
        cg += extra
        n_ins += sum(1 for op, _ in extra if op == "I")
    cg += [("M", 6)]
    return make_read(name, pos0, cg, seed=seed, mm=0.0, ins=[ins_base] * n_ins if ins_base else None, ref=ref)


def _terms_read(name, target, spacing, seed=0, min_del=2):
    """a read inside the long homopolymer with 1-base deletions `spacing` bases apart whose table needs exactly `target`
    terms when everything is tracked (every deletion's repeat run reaches the end of the read: nt = l_query - qpos + 1);
    net difference below the band switch, so that it stays in a register kernel or the wide one by its deletions alone"""
    for n_del in range(min_del, 40):
        for l_query in range(40, 280):
            for first in range(3, 2 * spacing + 3):      # the first deletion takes up the slack
                qs = [first] + [2 * spacing + 3 + spacing * k for k in range(n_del - 1)]
                if qs[-1] + 3 > l_query:
                    continue
                if sum(l_query - q + 1 for q in qs) == target:
                    cg, prev = [], 0
                    for q in qs:
                        cg += [("M", q - prev), ("D", 1)]
                        prev = q
                    cg.append(("M", l_query - prev))
                    r = make_read(name, HOMO_AT + 20, cg, seed=seed, mm=0.0)
                    assert HOMO_AT + 20 + l_query + n_del + 20 < HOMO_AT + HOMO_LEN
                    return r
    raise AssertionError("no deletion layout with %d terms" % target)


def boundary_table():
    t = []

    def add(name, kind, const, reads, routes, f_hi=None, overflow=False):
        assert kind in KINDS and len({r["name"] for r in reads}) == len(reads), name
        t.append(Row(name, kind, const, C[const][1], reads, routes, f_hi, overflow))

    R = REF_LEN
    # ---- read length: rows 1 .. 7 as the whole read, the stored-row parity, the batches of four of the backward sweep
    singles = [plain("len%d" % l, MID + 3 * i, l, seed=i) for i, l in enumerate(LENGTHS)]
    singles.insert(5, {"name": "len0", "pos0": MID, "cigar": [], "seq": np.zeros(0, np.uint8), "qual": np.zeros(0, np.uint8)})
    add("length: single reads, a zero-length read between two others", "length", "stored rows", singles, "narrow")
    for group in (LENGTHS[:8], LENGTHS[8:]):
        reads = []
        for L in group:                 # one whole wavefront per Lmax: lengths 1 .. L in turn, the longest in lane 37
            lens = [1 + (i * 7) % L for i in range(64)]
            lens[37] = L
            reads += _wave("max%d" % L, lens, seed=1000 * L)
        add("length: wavefront maxima Lmax = %s" % ", ".join(map(str, group)), "length", "batch clamp", reads, "narrow")
    # ---- interior range on / off: the wave minimum of fh on either side of BWF + 1
    full = _wave("p100", [100] * 64, at=300, seed=50)
    for l, f_hi in ((7, 0), (8, 0), (9, 8), (10, 9)):       # mid-contig: l_ref = l + 6, fh = l_ref - 7 = l - 1
        add("interior: one lane of %d bases among 100-base reads (fh %d)" % (l, l - 1), "interior", "f_hi",
            _swap(full, 17, plain("short%d" % l, MID, l, seed=l)), "narrow", f_hi=f_hi)
    for lr, f_hi in ((14, 0), (15, 8), (16, 9)):            # l_ref - 7 = 7, 8, 9 with l_query = l_ref + 7
        m = lr - 3
        reads = _swap(full, 5, make_read("clipL%d" % lr, 0, [("S", 10), ("M", m)], seed=lr))
        reads = _swap(reads, 40, make_read("clipR%d" % lr, R - m, [("M", m), ("S", 10)], seed=lr + 1))
        add("interior: one lane's window cut to l_ref %d by a contig end, l_query %d" % (lr, lr + 7), "interior", "fh",
            reads, "narrow", f_hi=f_hi)
    half = [plain("tiny%d" % i, 0, 1 + i % 3, seed=70 + i) for i in range(64)]    # l at pos0 0: l_ref = l + 3 = the band
    add("interior: one lane with bw < 7 among bw == 7 lanes", "interior", "fh",
        _swap(full, 63, plain("bw6", 0, 3, seed=3)), "narrow", f_hi=0)
    # ---- bw < 7: the window of a short read clipped by a contig end is shorter than the band
    ends = [plain("L%d" % l, 0, l, seed=l) for l in range(1, 7)] + [plain("R%d" % l, R - l, l, seed=10 + l) for l in range(1, 7)]
    add("bw < 7: reads of 1 to 6 bases at both contig ends", "bw<7", "b2", ends, "narrow")
    add("bw < 7: a whole wavefront of reads of 1 to 3 bases at pos0 0", "bw<7", "b2", half, "narrow", f_hi=0)
    # ---- l_ref 300 / 301: plain reads have l_ref = l + 6, a 1-base deletion gives l + 7
    lref = [plain("p294", 300, 294, seed=1), plain("p295", 302, 295, seed=2),
            make_read("d1_292", 304, "150M1D142M", seed=3), make_read("d1_293", 306, "150M1D143M", seed=4),
            make_read("d1_294", 308, "150M1D144M", seed=5),
            make_read("d2_291", 310, "150M2D141M", seed=6), make_read("d2_292", 312, "150M2D142M", seed=7),
            make_read("d2_293", 314, "150M2D143M", seed=8), plain("p295_pos0", 0, 295, seed=9)]
    lref_routes = ["narrow", "wide", "narrow", "narrow", "wide", "band8", "band8", "wide", "narrow"]
    add("l_ref 300 / 301: alone", "l_ref", "LFQ_BAQ_LDS_MAX_LREF", lref, lref_routes)
    mix = [plain("m150_%d" % i, 400 + 5 * i, 150, seed=30 + i) for i in range(12)]
    mixed = []
    for i, r in enumerate(lref):
        mixed += [mix[i], dict(r, name=r["name"] + "_mixed")]
    mixed += mix[len(lref):]
    add("l_ref 300 / 301: mixed with 150-base reads", "l_ref", "LFQ_BAQ_LDS_MAX_LREF", mixed,
        [x for rt in lref_routes for x in ("narrow", rt)] + ["narrow"] * (len(mix) - len(lref)))
    # ---- wr 51, 57, 63 and beyond
    widths, w_routes = [], []
    for d, rt_d, rt_i in ((1, "narrow", "narrow"), (2, "band8", "narrow"), (3, "band8", "narrow"), (5, "band8", "narrow"),
                          (6, "wide", "narrow"), (7, "wide", "narrow"), (8, "wide", "wide"), (9, "wide", "wide"),
                          (10, "wide", "wide")):
        widths += [make_read("del%d" % d, 320 + d, [("M", 60), ("D", d), ("M", 60)], seed=d),
                   make_read("ins%d" % d, 340 + d, [("M", 60), ("I", d), ("M", 60)], seed=20 + d)]
        w_routes += [rt_d, rt_i]
    widths.append(make_read("ins9_del9", 380, [("M", 40), ("I", 9), ("M", 40), ("D", 9), ("M", 40)], seed=41))
    w_routes.append("narrow")
    add("wr 51 / 57 / 63: deletions and insertions of 1 to 10 bases", "wr", "band switch", widths, w_routes)
    neighbours, n_routes = [], []
    for i in range(20):                 # a band-8 list that is smaller than a wavefront, between band-7 and wide reads
        d = (1, 2, 3, 6)[i % 4]
        neighbours.append(make_read("nb%d_del%d" % (i, d), 420 + 7 * i, [("M", 50 + i), ("D", d), ("M", 45)], seed=60 + i))
        n_routes.append(("narrow", "band8", "band8", "wide")[i % 4])
    add("wr 51 / 57 / 63: band-7, band-8 and wide deletions next to each other", "wr", "LFQ_BAQ_BAND8_CELLS", neighbours, n_routes)
    b8 = [make_read("b8_%d" % i, 330 + i, [("M", 40 + i % 30), ("D", 2 + i % 2), ("M", 50)], seed=80 + i) for i in range(70)]
    add("wr 57: more than a wavefront of band-8 reads", "wr", "LFQ_BAQ_BAND8_CELLS", b8, "band8")
    # ---- clips at the contig ends: the xb < 0 and xe > ref_len clamps make l_ref < l_query
    for side in ("leading", "trailing"):
        reads, routes = [], []
        for off in (0, 1):
            for s in range(1, 13):
                if side == "leading":
                    r = make_read("S%d_pos%d" % (s, off), off, [("S", s), ("M", 60)], seed=s + 20 * off)
                else:
                    r = make_read("S%d_end%d" % (s, off), R - off - 60, [("M", 60), ("S", s)], seed=s + 20 * off + 50)
                # the clamp leaves a window of 60 + 3 + off bases under a read of 60 + s
                cut = s - 3 - off
                reads.append(r)
                routes.append("narrow" if cut <= 7 else ("band8" if cut == 8 else "wide"))
        add("clips: %s soft clips of 1 to 12 at the contig %s" % (side, "start" if side == "leading" else "end"), "clips",
            "xb clamp" if side == "leading" else "xe clamp", reads, routes)
    # ---- IDAQ table edges
    hp = HOMO_AT
    edges = [make_read("ins16", MID, "50M16I50M", seed=1), make_read("ins17", MID + 2, "50M17I50M", seed=2),
             make_read("del16", MID + 4, "50M16D50M", seed=3), make_read("del17", MID + 6, "50M17D50M", seed=4),
             make_read("ins17_then_del2", MID + 8, "30M17I30M2D30M", seed=5),
             make_read("ins_first", MID + 10, "3I60M", seed=6), make_read("clip_then_del", MID + 12, "5S2D60M", seed=7),
             make_read("clip_then_ins", MID + 14, "5S2I60M", seed=8), make_read("ins_last", MID + 16, "60M3I", seed=9),
             make_read("del_first", MID + 18, "2D60M", seed=10), make_read("hardclip_then_del", MID + 19, "3H2D60M", seed=19),
             # the inserted A repeats to the end of the read: nt is cut at l_query
             make_read("ins_run_to_l_query", hp + 30, "20M1I30M", seed=11, mm=0.0, ins=["A"]),
             # the deleted A repeats to the end of the window: the scan stops at xe
             make_read("del_run_to_xe", hp + 40, "20M1D30M", seed=12, mm=0.0),
             make_read("del_run_to_contig_end", R - 52, "20M2D30M", seed=13),
             make_read("at_repeat_del2", AT_AT - 30, "32M2D40M", seed=14), make_read("at_repeat_ins2", AT_AT - 30, "32M2I40M", seed=15, ins=["AT"]),
             make_read("eq_x_ops", MID + 20, "20=1X20=2I10=1X10=3D20=", seed=16),
             make_read("over_n_ins", N_AT - 30, "28M2I40M", seed=17), make_read("lower_del", LOWER_AT - 20, "30M3D40M", seed=18)]
    add("idaq: indels of 16 and 17, first / last operations, the nt clamps, = and X", "idaq", "oplen skip", edges,
        ["wide", "wide", "wide", "wide", "wide", "narrow", "narrow", "narrow", "narrow", "narrow", "narrow", "narrow", "narrow",
         "narrow", "band8", "narrow", "narrow", "narrow", "band8"])
    add("idaq: exactly 64 indels, net difference 0", "idaq", "LFQ_BAQ_MAX_INDELS",
        [_indel_chain("chain64", MID, 32, seed=1)] + _wave("beside64", [90] * 63, at=320, seed=200), "narrow")
    add("idaq: 65 indels, net difference 0", "idaq", "LFQ_BAQ_MAX_INDELS",
        _swap(_wave("beside65", [90] * 64, at=320, seed=300), 31, _indel_chain("chain65", MID, 32, extra=[("I", 1), ("M", 2)], seed=2))
        + [_indel_chain("chain65_%d" % i, MID + 10 + i, 32, extra=[("I", 1), ("M", 2)], seed=3 + i) for i in range(63)]
        + [_indel_chain("chain66", MID + 5, 33, seed=90)], "narrow", overflow=True)
    t1024 = [_terms_read("terms1024", MAX_TERMS, 5, seed=1), _terms_read("terms1024_b", MAX_TERMS, 9, seed=2, min_del=8)]
    add("idaq: deletions in the homopolymer that need exactly 1024 terms", "idaq", "LFQ_BAQ_MAX_TERMS",
        t1024 + [make_read("hp_del_%d" % i, hp + 10 + i, [("M", 30 + i), ("D", 1), ("M", 40)], seed=400 + i, mm=0.0) for i in range(62)],
        [read_route_literal(r) for r in t1024] + ["narrow"] * 62)
    over = [_terms_read("terms%d" % n, n, 5, seed=n, min_del=md) for n, md in ((MAX_TERMS + 1, 2), (MAX_TERMS + 2, 8), (MAX_TERMS + 7, 2),
                                                                                (MAX_TERMS + 40, 9))]
    add("idaq: deletions in the homopolymer that need a few more than 1024 terms", "idaq", "LFQ_BAQ_MAX_TERMS",
        over + [make_read("hp_ins_%d" % i, hp + 10 + i, [("M", 30 + i), ("I", 1), ("M", 40)], seed=500 + i, mm=0.0, ins=["A"]) for i in range(60)],
        [read_route_literal(r) for r in over] + ["narrow"] * 60, overflow=True)
    clean = [make_read("idq%d" % i, 1450 + 4 * i, [("M", 30 + i % 20), ("ID"[i % 2], 1 + (i // 2) % 2 * (1 - i % 2)), ("M", 50)], seed=600 + i) for i in range(64)]
    add("idaq: a wavefront of indel reads without an N", "idaq", "nflag", clean, "narrow")
    with_n = [make_read("idqn%d" % i, N_AT - 70 + i, [("M", 30 + i % 20), ("I", 1 + i % 2), ("M", 50)], seed=700 + i) for i in range(64)]
    add("idaq: a wavefront of indel reads over the N of the contig", "idaq", "nflag", with_n, "narrow")
    # ---- quality values at the first, the last and an interior row
    quals = []
    for q in (0, 1, 2, 93, 255):
        for where, at in (("first", 0), ("interior", 47), ("last", 99)):
            qv = np.full(100, 30, np.uint8)
            qv[at] = q
            quals.append(plain("q%d_%s" % (q, where), MID + len(quals), 100, seed=800 + len(quals), qual=qv))
        quals.append(plain("q%d_all" % q, MID + len(quals), 33, seed=800 + len(quals), qual=q))
    add("quality: 0, 1, 2, 93 and 255 at the first, an interior and the last row", "quality", "quality table", quals, "narrow")
    return t


def read_route_literal(r):
    """the route of a homopolymer read whose deletions are all 1 base long: the net difference is their number n; the
    window is l_query + n + 6 wide before the trim (n <= 7; + 2 (n + 3) / 2 * 2 beyond), and the trim leaves a difference
    of 7 for n = 1 and 8 for n = 2 .. 5; everything else is wide -- as is any window beyond LFQ_BAQ_LDS_MAX_LREF"""
    n = sum(1 for op, _ in r["cigar"] if op == "D")
    l_ref = len(r["seq"]) + (7 if n == 1 else 8)
    if n > 5 or l_ref > MAX_LREF:
        return "wide"
    return "narrow" if n == 1 else "band8"


def row_routes(row):
    return [row.routes] * len(row.reads) if isinstance(row.routes, str) else list(row.routes)


def row_id(row):
    return re.sub(r"[^A-Za-z0-9]+", "_", row.name.replace("<", "lt").replace("==", "eq").replace("=", "eq")).strip("_")


def representatives(row, n):
    """at most n reads of the row for the binary's fixture: one per distinct (route, band, length, CIGAR operations, extreme qualities), spread
    evenly over the row where there are more than n of those"""
    seen, keep = set(), []
    for r in row.reads:
        g = read_geometry(r, REF_LEN)
        key = (g.route, g.b2, len(r["seq"]), "".join(op for op, _ in r["cigar"]), bytes(sorted(set(r["qual"][r["qual"] < 3]))),
               int(r["qual"].max(initial=0)) > 41)
        if key not in seen:
            seen.add(key)
            keep.append(r)
    if len(keep) > n:               # the last read of every route stays (the one nearest the boundary in most rows)
        route = lambda r: read_geometry(r, REF_LEN).route
        must = {route(r): i for i, r in enumerate(keep)}
        idx = set(must.values())
        rest = [i for i in range(len(keep)) if i not in idx]
        m = n - len(idx)
        idx |= {rest[(k * (len(rest) - 1)) // max(m - 1, 1)] for k in range(m)}
        keep = [keep[i] for i in sorted(idx)]
    return keep
