"""Contigs and read sets at the geometry boundaries of the indelqual kernels (lofreq_amd/csrc/lfq_indelqual.hip).

  lfq_idq_table_kernel  tiles of LFQ_IDQ_TILE positions counted from tab_begin = (lowest matched position) / 16 * 16, 16
                        positions a lane, LFQ_IDQ_HALO bytes staged behind a tile, a backward run-length pass that saturates
                        at 19.  A row chooses tab_begin by its lowest read, and with it where the tile edges fall: every
                        contig holds a series of sites, 48 bases apart, each with a run planted around the first and the
                        second tile edge of its own tab_begin; the lane edges (multiples of 16) are the same for every row.
  lfq_idq_fill_kernel   a lane owns 16 aligned output bytes, whichever reads they belong to: read sets whose reads, zero-length
                        reads and I / S / D operations fall on those chunk edges, and whose n_bases sits on a chunk and on a
                        block edge.

The reference is tests/indelqual_model.py; tests/golden/indelqual_edges.json holds what `lofreq indelqual --dindel` of the
2.1.4 binary wrote for every read with bases (main() below, through tests/make_indelqual_golden.py: run_family).

    python tests/indelqual_edges.py          (LFQ_GOLDEN_OUT: another output directory)
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
import indelqual_model as im  # noqa: E402

SRC = os.path.join(ROOT, "lofreq_amd", "csrc", "lfq_indelqual.hip")
FIXTURE = os.path.join(HERE, "golden", "indelqual_edges.json")
UNIFORM = "u40,25"


def source_constants():
    text = open(SRC).read()

    def find(pattern):
        m = re.search(pattern, text)
        assert m, "lfq_indelqual.hip: nothing matches %r" % pattern
        return [int(v) for v in m.groups()]
    c = {}
    c["TILE"], = find(r"#define\s+LFQ_IDQ_TILE\s+(\d+)\b")
    c["HALO"], = find(r"#define\s+LFQ_IDQ_HALO\s+(\d+)\b")
    c["SAT"], = find(r"run = same \? min\(run \+ 1, (\d+)\) : 1;")
    c["LANE"], = find(r"const int64_t x0 = tile0 \+ \(int64_t\)t \* (\d+);")
    c["CHUNK"], = find(r"const int64_t b0 = chunk \* (\d+);")
    threads, = find(r"const int64_t chunk = \(int64_t\)blockIdx\.x \* (\d+) \+ threadIdx\.x;")
    c["BLOCK"] = threads * c["CHUNK"]                                   # output bytes of one block of the fill kernel
    assert find(r"return \(uint8_t\)\(count > (\d+) \? '!'") == [c["SAT"] - 1] and len(im.DINDELQ) == c["SAT"]
    assert re.search(r"if \(x > ref_len - 2\) \{", text) and c["TILE"] == threads * c["LANE"] and c["HALO"] >= c["SAT"]
    return c


C = source_constants()
TILE, HALO, SAT, LANE, CHUNK, BLOCK = (C[k] for k in ("TILE", "HALO", "SAT", "LANE", "CHUNK", "BLOCK"))

# ---- the contigs ------------------------------------------------------------------------------------------------------

RUN_LENGTHS = (1, 2, SAT - 2, SAT - 1, SAT, SAT + 1, 25)
END_LENGTHS = (2, SAT - 1, SAT, SAT + 1)
SITE_STEP = 3 * LANE                    # distance of two sites: a run of 25 and its guards fit
FIRST_BEGIN = 10 * LANE                 # tab_begin of site 0
LANES_AT = 2000                         # the region of the lane-edge runs, below every first tile edge
REF_LENS = (9008, 9009, 9007)           # modulo 16: 0, 1, 15; more than two tiles with a partial last one


def edge_plants():
    """what is planted around a tile edge E, one per site: (kind, start - E, length)"""
    p = [("start", off, L) for L in RUN_LENGTHS for off in (-1, 0, 1)]
    p += [("end", endoff - L + 1, L) for L in END_LENGTHS for endoff in (-1, 0)]
    p += [("N", -3, 6), ("lower", -4, 10), ("mixed", -9, SAT)]
    return p


def lane_plants():
    """around a lane edge E (a multiple of 16): (kind, start - E, length); a start at -1 / 0 is offset 15 of one lane's 16
    positions / offset 0 of the next, what the issue calls offset 16"""
    p = [("start", off, L) for L in RUN_LENGTHS for off in (-1, 0)]
    p += [("end", endoff - L + 1, L) for L in END_LENGTHS for endoff in (-1, 0)]
    p += [("lower", -4, 8)]
    return p


def _plant(g, start, L, kind, k):
    letter = "N" if kind == "N" else "ACGT"[k % 4]
    g[start:start + L] = letter * L
    for p in (start - 1, start + L):
        if 0 <= p < len(g):
            g[p] = "ACGT"[(k + 1 + (p > start)) % 4]        # the run is exactly L long
    return letter


def make_contigs():
    """-> ({name: sequence}, {name: [site]}, {name: [lane plant]}); site = dict(tab_begin, plants [(edge number, kind, start, L)])"""
    contigs, sites, lanes = {}, {}, {}
    ep, lp = edge_plants(), lane_plants()
    per = (len(ep) + len(REF_LENS) - 1) // len(REF_LENS)
    for ci, ref_len in enumerate(REF_LENS):
        name = "c%d" % (ref_len % LANE)
        rng = np.random.default_rng(8900 + ci)
        g = list(rng.choice(list("ACGT"), ref_len))
        sites[name], lanes[name] = [], []
        for s in range(per):
            k = ci * per + s
            tab_begin = FIRST_BEGIN + SITE_STEP * s
            plants = []
            for e, (kind, off, L) in ((1, ep[k % len(ep)]), (2, ep[(k + len(ep) // 2) % len(ep)])):
                start = tab_begin + e * TILE + off
                letter = _plant(g, start, L, kind, k + e)
                edge = tab_begin + e * TILE
                if kind == "lower":
                    g[edge - 1], g[edge] = letter.lower(), letter.lower()
                if kind == "mixed":
                    g[edge] = letter.lower()
                plants.append((e, kind, start, L))
            sites[name].append({"tab_begin": tab_begin, "plants": plants})
        for j, (kind, off, L) in enumerate(lp):
            edge = LANES_AT + SITE_STEP * (j + 1)
            letter = _plant(g, edge + off, L, kind, j + ci)
            if kind == "lower":
                g[edge - 1], g[edge] = letter.lower(), letter.lower()
            lanes[name].append((kind, edge + off, L))
        # the contig's end: a run that ends on the last base, one that ends one base before it, one of 25 that the end cuts
        if ci == 0:
            g[ref_len - 6], g[ref_len - 5:] = "A", "C" * 5
        elif ci == 1:
            g[ref_len - SAT - 1], g[ref_len - SAT:ref_len - 1], g[ref_len - 1] = "C", "G" * (SAT - 1), "A"
        else:
            g[ref_len - 26], g[ref_len - 25:] = "T", "G" * 25
        contigs[name] = "".join(g)
    return contigs, sites, lanes


CONTIGS, SITES, LANE_PLANTS = make_contigs()


# ---- reads and rows ---------------------------------------------------------------------------------------------------

def rd(name, pos0, cigar):
    cigar = [(o, int(l)) for l, o in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    lq = sum(l for o, l in cigar if o in "MIS=X")
    return {"name": name, "pos0": int(pos0), "cigar": cigar, "l_qseq": lq, "seq": "A" * lq, "qual": [30] * lq}


def empty(name, pos0):
    return rd(name, pos0, "")


Row = namedtuple("Row", "name kind contig reads")
KINDS = ("tile", "lanes", "reads", "ops", "n_bases")
Geom = namedtuple("Geom", "lo hi tab_begin tab_end edges n_bases seq_off")


def geometry(row):
    """the span of the table as lfq_readset_indelqual computes it, the tile edges inside it, and the seq_off layout"""
    ref_len = len(CONTIGS[row.contig])
    lo, hi = None, 0
    for r in row.reads:
        x = r["pos0"]
        for op, l in r["cigar"]:
            if op in "M=X" and l > 0:
                lo = x if lo is None else min(lo, x)
                hi = max(hi, x + l)
            x += l if op in "M=XD" else 0
    tab_begin, tab_end = lo // LANE * LANE, min(hi, ref_len)
    seq_off = np.cumsum([0] + [r["l_qseq"] for r in row.reads])
    return Geom(lo, hi, tab_begin, tab_end, list(range(tab_begin + TILE, tab_end, TILE)), int(seq_off[-1]), [int(v) for v in seq_off])


def chunk_owners(row):
    """per 16-byte chunk of the output: the indices of the reads with a byte in it"""
    g = geometry(row)
    out = []
    for b0 in range(0, g.n_bases, CHUNK):
        out.append([i for i in range(len(row.reads)) if g.seq_off[i] < min(b0 + CHUNK, g.n_bases) and g.seq_off[i + 1] > b0])
    return out


def boundary_table():
    t = []

    def add(name, kind, contig, reads):
        assert kind in KINDS and len({r["name"] for r in reads}) == len(reads), name
        assert [r["pos0"] for r in reads] == sorted(r["pos0"] for r in reads), name        # a read set is sorted
        t.append(Row(name, kind, contig, reads))

    # ---- the table kernel: one row per site, whose lowest read sets tab_begin and with it the tile edges
    n = 0
    for contig in CONTIGS:
        ref_len = len(CONTIGS[contig])
        for s, site in enumerate(SITES[contig]):
            b = site["tab_begin"]
            m = (0, 1, LANE - 1)[n % 3]
            e1, e2 = b + TILE, b + 2 * TILE
            end = (("last", ref_len - 40), ("before", ref_len - 41), ("past", ref_len - 34))[(n // 3) % 3]
            reads = [rd("lo%d" % m, b + m, "20M"), rd("e1", e1 - 70, "150M"), rd("e1_del", e1 - 40, "30M5D60M"),
                     rd("e1_eqx", e1 - 30, "2S25=2X1I40="), rd("e2", e2 - 70, "150M"), rd("e2_ins", e2 - 35, "30M2I60M"),
                     rd("end_" + end[0], end[1], "40M")]
            what = "; ".join("%s of %d at edge %d %+d" % (k, L, e, st - (b + e * TILE)) for e, k, st, L in site["plants"])
            add("tile %s site %d: lo %% 16 = %d, %s, read %s" % (contig, s, m, what, end[0]), "tile", contig, reads)
            n += 1
    for contig in CONTIGS:
        last = LANES_AT + SITE_STEP * (len(LANE_PLANTS[contig]) + 2)
        reads = [rd("lane%d" % p, p, "150M") for p in range(LANES_AT - 30, last, 140)]
        add("lanes %s: runs that start and end on lane edges" % contig, "lanes", contig, reads)
    # ---- the fill kernel
    c = "c0"
    lens = list(range(1, 18)) + [6] * 8 + list(range(17, 0, -1))
    add("reads of 1 to 17 bases: chunks with three, four and more reads", "reads", c,
        [rd("s%d" % i, 301 + 3 * i, "%dM" % l) for i, l in enumerate(lens)])
    add("zero-length reads first, last and between reads", "reads", c,
        [empty("z0", 300), rd("a", 303, "7M"), empty("z1", 305), empty("z2", 305), rd("b", 306, "9M"), rd("c", 310, "3S12M2I8M"),
         empty("z3", 311), rd("d", 312, "21M"), empty("z4", 330)])
    add("only zero-length reads around one base", "reads", c, [empty("z0", 319), rd("a", 319, "1M"), empty("z1", 320)])
    add("a chunk edge before, inside and after an I, an S and a D", "ops", c,
        [rd("i_before", 335, "16M2I14M"), rd("i_inside", 336, "15M2I15M"), rd("i_after", 337, "14M2I16M"),
         rd("s_after", 338, "14M2S"), rd("s_before", 339, "2S14M"), rd("m15", 340, "15M"), rd("s_inside", 341, "2S15M"),
         rd("d_on", 342, "16M3D16M"), rd("d_before", 343, "15M3D17M"), rd("d_after", 344, "17M3D15M"), rd("s_tail_inside", 345, "15M2S15H")])
    for nb in (3 * CHUNK, 3 * CHUNK + 1, 3 * CHUNK - 1):
        add("n_bases %d" % nb, "n_bases", c, [rd("a", 351, "20M"), rd("b", 352, "10M1D%dM" % (nb - 30))])
    for nb in (BLOCK, BLOCK + 1):
        k = nb // 150
        add("n_bases %d" % nb, "n_bases", c, [rd("r%d" % i, 365 + 7 * i, "150M") for i in range(k)] + [rd("rest", 365 + 7 * k, "%dM" % (nb - 150 * k))])
    assert len({row_id(r) for r in t}) == len(t)
    return t


def row_id(row):
    return re.sub(r"[^A-Za-z0-9]+", "_", row.name.split(":")[0]).strip("_")


def model_strings(row):
    table = im.dindel_table(CONTIGS[row.contig])
    return [im.dindel_read(table, r["pos0"], r["cigar"]) for r in row.reads]


# ---- the fixture ------------------------------------------------------------------------------------------------------

def load_fixture():
    return json.load(open(FIXTURE))


def inline_read(r):
    return [r["name"], r["pos0"], "".join("%d%s" % (l, o) for o, l in r["cigar"]), r["l_qseq"]]


def main():
    import make_indelqual_golden as mg
    fix = {"name": "indelqual_edges", "generator": "tests/indelqual_edges.py", "reference_binary": "lofreq 2.1.4 (dist tgz)",
           "command": "lofreq indelqual --dindel -f t.fa -o out.bam t.sam", "contigs": CONTIGS, "rows": []}
    for row in boundary_table():
        asked = [r for r in row.reads if r["l_qseq"] > 0]         # a record without bases is none the command can be given
        _, res = mg.run_family(CONTIGS[row.contig], asked)
        assert res["dindel"]["bd"] is None
        bi = iter(res["dindel"]["bi"])
        fix["rows"].append({"name": row.name, "contig": row.contig, "reads": [inline_read(r) for r in row.reads],
                            "bi": [next(bi) if r["l_qseq"] > 0 else None for r in row.reads]})
    mg.dump("indelqual_edges", fix)


if __name__ == "__main__":
    main()
