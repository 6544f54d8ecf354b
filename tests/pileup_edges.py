"""Reads at the row, round and tile boundaries of the read-level pileup's tile kernels (lfq_pileup.hip:
lfq_pileup_tiles_kernel<false, 256> / <true, 128>, lfq_plp_indel_tiles_kernel, lfq_plp_indel_columns_kernel<true>, the nt packing).

Used by test_pileup_edges.py (CPU: the two resolvers restated, a numpy model of the fast path, the two references against
each other) and test_gpu_pileup_edges.py (every row on the device, against the references):

  constants       LFQ_TILE, LFQ_TILE_ROW, the reads per round of the three kernels and the event cap, read from the source;
  read            one read dict with reproducible bytes;
  boundary_table  the rows: name, group, reads, ref, region, gates and what the marked read does in the marked tile.

A claim is written down from how the row was built -- the stretch lengths, the alignment asked for -- and never by running a
resolver: test_pileup_edges.py holds it against the restated resolvers.

A row's claims (one per marked tile of the marked read):
  read        index of the marked read in the row's sorted reads
  tile        index of the marked tile: positions begin + tile * LFQ_TILE ...
  a           g0 & 15, g0 = seq_off[read] + the query index of the read's first base in the tile (None: no base there, or more
              than two stretches -- the resolvers compute no row then)
  nseg        stretches of the query the tile's positions map to, as lfq_tile_resolve counts them
  nw          16-byte words the SNV resolver fetches per track (0: none, or the slow path)
  slow        the SNV resolver goes position by position
  slow_indel  the indel resolver does
  nev         positions of the tile an insertion or deletion follows
  tail_dp     the read's last aligned position if it is a covered one of this tile, else 255
  off1_neg    (some rows) the second stretch's row offset is negative
Rows of the group `round` claim the number of reads in the marked tile's window, rows of the group `region` the tiles of the
region and the width of the last.

No test in here."""
import os
import re
import zlib
from collections import namedtuple

import numpy as np

import bam_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "lofreq_amd/csrc/lfq_pileup.hip"


# ---- the constants, read from the source ----------------------------------------------------------------------------------

def _source_int(pattern, count=1):
    """the integer groups of the only line(s) of the source that match `pattern`; anything but `count` matches is an error"""
    with open(os.path.join(ROOT, SRC)) as f:
        found = [(m, i) for i, line in enumerate(f, 1) for m in [re.search(pattern, line)] if m]
    assert len(found) == count, "%s: %d lines match %r, expected %d" % (SRC, len(found), pattern, count)
    return [tuple(int(x) for x in m.groups()) for m, _ in found]


TILE = bam_records.source_constant("LFQ_TILE", SRC)                 # positions per workgroup
ROW = bam_records.source_constant("LFQ_TILE_ROW", SRC)              # bytes of LDS per read and track
WORDS = ROW // 16                                                   # aligned 16-byte words a row holds
CAP = WORDS * 16                                                    # (g0 & 15) + span <= CAP: the fast path
RC_SCATTER = _source_int(r"\(lfq_pileup_tiles_kernel<true, (\d+)>\), grid, block")[0][0]
RC_COUNT = _source_int(r"\(lfq_pileup_tiles_kernel<false, (\d+)>\), grid, block")[0][0]
RC_INDEL = _source_int(r"^    constexpr int RC = (\d+);")[0][0]
EV_CAP = _source_int(r"\|\| nev > (\d+) \|\|")[0][0]                 # events per read and tile the indel resolver keeps
assert _source_int(r"^    int ev_dp\[(\d+)\], ev_val\[(\d+)\];")[0] == (EV_CAP, EV_CAP)
SLICE = 64                                                          # reads per phase-B slice: a wavefront
R = min(RC_SCATTER, RC_INDEL)                                       # the smaller round
assert R % SLICE == 0 and RC_COUNT % R == 0 and CAP >= TILE + 16 and TILE == 64

NO_TAIL = 255
OPS = "MIDNSHP=X"


# ---- reads ------------------------------------------------------------------------------------------------------------------

def parse(cigar):
    out = [(m.group(2), int(m.group(1))) for m in re.finditer(r"(\d+)([%s])" % OPS, cigar)]
    assert "".join("%d%s" % (l, o) for o, l in out) == cigar, cigar
    return out


def _seed(name):
    return zlib.crc32(name.encode())


def read(pos0, cigar, seed, mark=False, **over):
    """a read dict: seq codes 0..3, qualities 10..41, lb / bi / bd bytes, mapq, strand -- all from `seed`; `over` replaces
    entries: an array, None (the read has no such tag), or a function of the query length"""
    cig = parse(cigar)
    ql = sum(l for o, l in cig if o in "MIS=X")
    rng = np.random.default_rng(seed)
    d = {"pos0": int(pos0), "cigar": cig, "seq": rng.integers(0, 4, ql).astype(np.uint8),
         "qual": rng.integers(10, 42, ql).astype(np.uint8), "mapq": int(rng.integers(1, 61)), "reverse": bool(rng.integers(0, 2)),
         "lb": rng.integers(34, 100, ql).astype(np.uint8), "bi": (33 + rng.integers(10, 50, ql)).astype(np.uint8),
         "bd": (33 + rng.integers(10, 50, ql)).astype(np.uint8)}
    for k, v in over.items():
        d[k] = v(ql) if callable(v) else v
    for k in ("seq", "qual", "lb", "bi", "bd"):
        if d[k] is not None:
            d[k] = np.asarray(d[k], np.uint8)
            assert len(d[k]) == ql, (k, cigar)
    if mark:
        d["mark"] = True
    return d


def ref_end(r):
    return r["pos0"] + sum(l for o, l in r["cigar"] if o in "MDN=X")


def seq_offsets(reads):
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r["seq"]) for r in reads])
    return off


def cycle(values):
    return lambda ql: np.asarray(values)[np.arange(ql) % len(values)]


def make_ref(n, seed):
    return "".join("ACGT"[c] for c in np.random.default_rng(seed).integers(0, 4, n))


Row = namedtuple("Row", "name group reads ref begin end min_plp_bq min_plp_idq claim")

REF = make_ref(1024, 11)
MT = 2                                                              # the marked tile of the groups `row` and `round`
P0 = MT * TILE                                                      # ... its first position (begin = 0)
ROW_END = 5 * TILE + 7                                              # the region of those groups ends inside a tile


def _background(seed):
    """plain reads around the marked tile, and one with an insertion and a deletion: its two columns with an event are where
    the indel pileup lists every read WITHOUT one, in pileup order"""
    return [read(P0 - 50, "90M", seed + 1), read(P0 - 30, "50M1I30M2D20M", seed + 2), read(P0 - 3, "40M", seed + 3),
            read(P0 + 20, "70M", seed + 4), read(P0 + 50, "60M", seed + 5)]


def place(reads, q1, a):
    """the reads sorted by start, behind a read at position 0 whose length puts (seq_off[marked read] + q1) & 15 at `a`
    -> (reads, index of the marked read)"""
    reads = sorted(reads, key=lambda r: r["pos0"])
    (i,) = [k for k, r in enumerate(reads) if r.get("mark")]
    g0 = int(seq_offsets(reads)[i]) + q1
    k = (a - g0) % 16 or 16
    return [read(0, "%dM" % k, 99)] + reads, i + 1


def claim(tile, a, nseg, span, nev, tail_dp, slow_indel=False, **extra):
    """what the resolvers make of `nseg` stretches spanning `span` query bytes that start at alignment a"""
    nw = (a + span + 15) // 16 if nseg in (1, 2) else 0
    slow = nseg > 2 or nw > WORDS
    return dict(tile=tile, a=a if nseg in (1, 2) else None, nseg=nseg, nw=0 if slow else nw, slow=slow,
                slow_indel=bool(slow_indel or slow or nev > EV_CAP or nseg == 0), nev=nev, tail_dp=tail_dp, **extra)


def _row(t, name, pos, cigar, q1, a, claims, min_plp_bq=3, min_plp_idq=0, bg_over=None, no_lb=False, **over):
    """a row of the group `row`: the marked read among the background reads.  claims: [(tile, query index of the read's first
    base in it, nseg, span, nev, tail_dp[, slow_indel[, extra]])], the first tile being the one `a` is set for"""
    seed = _seed(name)
    bg = _background(seed)
    for k, o in (bg_over or {}).items():
        bg[k] = read(bg[k]["pos0"], "".join("%d%s" % (l, op) for op, l in bg[k]["cigar"]), seed + 1 + k, **o)
    reads, i = place(bg + [read(pos, cigar, seed, mark=True, **over)], q1, a)
    if no_lb:
        for r in reads:
            r["lb"] = None
    out = []
    for c in claims:
        tile, q, nseg, span, nev, tail = c[:6]
        d = claim(tile, (a + q - q1) % 16, nseg, span, nev, tail, c[6] if len(c) > 6 else False, **(c[7] if len(c) > 7 else {}))
        out.append(dict(d, read=i))
    assert all(ref_end(r) <= len(REF) for r in reads)
    t.append(Row("row/" + name, "row", reads, REF, 0, ROW_END, min_plp_bq, min_plp_idq, tuple(out)))


ALIGNMENTS = (0, 1, 15)


def _row_rows(t):
    H = TILE // 2
    for a in ALIGNMENTS:
        # one stretch of a whole tile: 4 words at a = 0, else 5; one base: 1 word
        _row(t, "one_stretch/a%d" % a, P0, "%dM" % TILE, 0, a, [(MT, 0, 1, TILE, 0, TILE - 1)])
        _row(t, "one_base/a%d" % a, P0 + 17, "1M", 0, a, [(MT, 0, 1, 1, 0, 17)])
        # a whole tile and one insertion: a + TILE + L bytes of the query; CAP of them fit the row
        for L in (CAP - TILE - a, CAP - TILE - a + 1):
            _row(t, "ins_capacity/a%d/L%d" % (a, L), P0, "%dM%dI%dM" % (H, L, H), 0, a, [(MT, 0, 2, TILE + L, 1, TILE - 1)])
    # a deletion instead: the second stretch's offset a + (q2 - q1) - p2 is negative
    _row(t, "deletion/dlen1", P0, "%dM1D%dM" % (H, H - 1), 0, 0, [(MT, 0, 2, TILE - 1, 1, TILE - 1, False, dict(off1_neg=True))])
    for a in (0, 15):
        _row(t, "deletion/dlen%d/a%d" % (TILE - 2, a), P0, "1M%dD1M" % (TILE - 2), 0, a,
             [(MT, 0, 2, 2, 1, TILE - 1, False, dict(off1_neg=True))])
    # = X M next to each other: one stretch; an I between them: two
    _row(t, "join/eq_X_M", P0 + 5, "10=1X20M", 0, 1, [(MT, 0, 1, 31, 0, 35)])
    _row(t, "join/eq_I_X_M", P0 + 5, "10=3I1X20M", 0, 1, [(MT, 0, 2, 34, 1, 35)])
    # two indels in one tile: three stretches.  The same two a tile apart: two stretches in each of two tiles
    _row(t, "join/two_indels_one_tile", P0 + 5, "10M2I10M3D10M", 0, 1, [(MT, 0, 3, 0, 2, 37)])
    _row(t, "join/two_indels_a_tile_apart", P0 + 5, "10M2I%dM3D10M" % TILE, 0, 1,
         [(MT, 0, 2, 12 + TILE - 15, 1, NO_TAIL), (MT + 1, 12 + TILE - 15, 2, 25, 1, 27)])
    # indels at the tile edge
    _row(t, "edge/ins_after_last_dp", P0, "%dM5I20M" % TILE, 0, 15, [(MT, 0, 1, TILE, 1, NO_TAIL), (MT + 1, TILE + 5, 1, 20, 0, 19)])
    _row(t, "edge/del_then_M_at_last_dp", P0, "%dM2D10M" % (TILE - 3), 0, 15,
         [(MT, 0, 2, TILE - 2, 1, NO_TAIL), (MT + 1, TILE - 2, 1, 9, 0, 8)])
    _row(t, "edge/del_reaches_tile_end", P0, "%dM2D10M" % (TILE - 2), 0, 15,
         [(MT, 0, 1, TILE - 2, 1, NO_TAIL, True), (MT + 1, TILE - 2, 1, 10, 0, 9)])
    _row(t, "edge/del_from_previous_tile_ends_dp0", P0 - 10, "8M3D20M", 8, 1,
         [(MT, 8, 1, 20, 0, 20), (MT - 1, 0, 1, 8, 1, NO_TAIL, True)])
    _row(t, "edge/del_from_previous_tile_ends_dp5", P0 - 10, "8M8D20M", 8, 1,
         [(MT, 8, 1, 20, 0, 25), (MT - 1, 0, 1, 8, 1, NO_TAIL, True)])
    # a tile wholly inside a deletion / a skip
    for op in "DN":
        _row(t, "edge/tile_inside_%s" % op, P0 - 20, "10M%d%s10M" % (2 * TILE + 12, op), 10, 1,
             [(MT, 0, 0, 0, 0, NO_TAIL, True), (MT - 1, 0, 1, 10, 1 if op == "D" else 0, NO_TAIL, True),
              (MT + 2, 10, 1, 10, 0, 11)])
    # what follows a deletion
    _row(t, "after_del/D_I", P0 + 2, "20M2D3I20M", 0, 1, [(MT, 0, 2, 43, 2, 43, True)])
    _row(t, "after_del/D_N", P0 + 2, "20M2D5N20M", 0, 1, [(MT, 0, 2, 40, 1, 48, True)])
    _row(t, "after_del/D_S", P0 + 2, "20M2D4S", 0, 1, [(MT, 0, 1, 20, 1, NO_TAIL, True)])
    _row(t, "after_del/D_last", P0 + 2, "20M2D", 0, 1, [(MT, 0, 1, 20, 1, NO_TAIL, True)])
    _row(t, "after_del/M_P_I_M", P0 + 2, "20M1P2I20M", 0, 1, [(MT, 0, 2, 42, 1, 41)])
    # clips
    _row(t, "clip/leading_S", P0 + 3, "7S30M", 7, 15, [(MT, 7, 1, 30, 0, 32)])
    _row(t, "clip/leading_H", P0 + 3, "5H30M", 0, 15, [(MT, 0, 1, 30, 0, 32)])
    _row(t, "clip/trailing_S_H", P0 + 3, "30M6S3H", 0, 15, [(MT, 0, 1, 30, 0, 32)])
    # EV_CAP events and one more.  (An event needs a stretch to end: a read with EV_CAP of them in a tile has more than two
    # stretches there, which the resolvers flag on their own.)
    assert EV_CAP == 3
    _row(t, "events/3", P0, "10M1I10M1D10M2I10M", 0, 1, [(MT, 0, 4, 0, 3, 40)])
    _row(t, "events/3_last_at_dp%d" % (TILE - 1), P0 + TILE - 40, "10M1I10M1D19M2I10M", 0, 1,
         [(MT, 0, 3, 0, 3, NO_TAIL), (MT + 1, 42, 1, 10, 0, 9)])
    _row(t, "events/4", P0, "8M1I8M1D8M2I8M2D8M", 0, 1, [(MT, 0, 5, 0, 4, 42)])
    # the read's last aligned position
    _row(t, "tail/at_dp0", P0 - 20, "21M", 20, 1, [(MT, 20, 1, 1, 0, 0)])
    _row(t, "tail/at_last_dp", P0 + 10, "%dM" % (TILE - 10), 0, 1, [(MT, 0, 1, TILE - 10, 0, TILE - 1)])
    _row(t, "tail/M_then_I", P0, "30M4I", 0, 1, [(MT, 0, 1, 30, 1, 29)])
    _row(t, "tail/M_then_S", P0, "30M5S", 0, 1, [(MT, 0, 1, 30, 0, 29)])
    _row(t, "tail/ends_in_D", P0, "30M3D", 0, 1, [(MT, 0, 1, 30, 1, NO_TAIL, True)])
    # the gates and the bytes
    whole = [(MT, 0, 1, TILE, 0, TILE - 1)]
    _row(t, "bytes/bq_gate", P0, "%dM" % TILE, 0, 1, whole, min_plp_bq=20, qual=cycle([19, 20, 20, 19, 19]),
         bg_over={0: dict(qual=cycle([20, 19])), 3: dict(qual=cycle([19, 19, 20]))})
    _row(t, "bytes/bq_cap", P0, "%dM" % TILE, 0, 1, whole, qual=cycle([93, 94, 255, 40, 2, 3]))
    _row(t, "bytes/lb", P0, "%dM" % TILE, 0, 1, whole, lb=cycle([32, 33, 126, 60, 0, 255, 34]))
    _row(t, "bytes/no_lb", P0, "%dM" % TILE, 0, 1, whole, no_lb=True)
    _row(t, "bytes/base_codes", P0, "%dM" % TILE, 0, 1, whole, seq=cycle(list(range(4, 16)) + [0, 1, 2, 3]))
    idq = [(MT, 0, 2, TILE - 1, 1, TILE - 1, False, dict(off1_neg=True))]
    _row(t, "bytes/idq_gate", P0, "%dM1D%dM" % (H, H - 1), 0, 0, idq, min_plp_idq=20,
         bi=cycle([33 + 19, 33 + 20, 33 + 20]), bd=cycle([33 + 20, 33 + 20, 33 + 19, 33 + 20, 33 + 20]),
         bg_over={0: dict(bi=None), 2: dict(bd=None), 3: dict(bi=None, bd=None), 4: dict(bi=cycle([33 + 19, 33 + 20]))})


# ---- deep piles: the rounds and slices ----------------------------------------------------------------------------------------

ROUND_N = (R // 2 - 1, R // 2, R // 2 + 1, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 3 * R + 1)
ROUND_BQ, ROUND_IDQ = 13, 15


def _pile_read(i, pos):
    """read i of a pile: kept and dropped bases alternate with the read and the position, so that a kept base's rank in its
    column depends on every read before it; (mapq, kept quality) is different for every read, and so are its BI / BD bytes"""
    cigar = "44M1I36M" if i % 16 == 3 else "20M2D58M" if i % 16 == 11 else "80M"

    def qual(ql):
        j = np.arange(ql)
        return np.where((i * 5 + j * 3 + (i >> 6)) % 7 < 4, 20 + i % 37, ROUND_BQ - 1 - i % 2)

    def tag(mul):
        return lambda ql: 33 + 10 + (i * mul + np.arange(ql)) % 12           # 10 .. 21, the gate is 15
    return read(pos, cigar, 1000 + i, mapq=i % 254, reverse=bool((i // 3) % 2), qual=qual, bi=tag(7), bd=tag(5))


def _round_rows(t):
    assert set(ROUND_N) >= {SLICE - 1, SLICE, SLICE + 1, RC_SCATTER, RC_SCATTER + 1, RC_INDEL + 1, RC_COUNT - 1, RC_COUNT, RC_COUNT + 1}
    for n in ROUND_N:
        reads = [_pile_read(i, P0 - 8) for i in range(n)]
        t.append(Row("round/n%d" % n, "round", reads, REF, 0, 4 * TILE, ROUND_BQ, ROUND_IDQ, (dict(tile=MT, window=n),)))
    # a long first read that reaches the tile, reads that end before it, then the pile: a slice / a round of the window with
    # no overlap
    for what, shorts in (("slice", 2 * SLICE - 1), ("round", 2 * R - 1)):
        reads = [read(P0 - 100, "120M", 7)]
        reads += [read(P0 - 99 + (90 * k) // shorts, "5M", 2000 + k) for k in range(shorts)]
        reads += [_pile_read(i, P0 - 8) for i in range(SLICE + 6)]
        assert len(reads) <= 600 and all(ref_end(r) <= P0 for r in reads[1:1 + shorts])
        t.append(Row("round/empty_%s" % what, "round", reads, REF, 0, 4 * TILE, ROUND_BQ, ROUND_IDQ,
                     (dict(tile=MT, window=len(reads), empty=what),)))


# ---- regions ----------------------------------------------------------------------------------------------------------------

REGION_REF = make_ref(512, 12)
REGION_WIDTHS = (1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1)
REGION_BEGINS = (0, 1, TILE - 1, TILE)
GAP = (200, 230)                                                    # no read of the pile covers these positions


def region_pile():
    """about 40 ragged reads over positions 0 .. 400, none over GAP"""
    rng = np.random.default_rng(31)
    starts = [0, 0, 1, TILE - 1, TILE, 100, 101, 110, 2 * TILE - 1, 2 * TILE]
    starts += rng.integers(0, 160, 14).tolist() + rng.integers(GAP[1], 360, 16).tolist()
    shapes = ("%dM", "%dM", "%dM", "5M2I%dM", "6M3D%dM", "4S%dM", "3=1X%dM", "%dM3S")
    reads = []
    for k, s in enumerate(sorted(starts)):
        n = int(rng.integers(5, 30))
        reads.append(read(s, shapes[k % len(shapes)] % n, 3000 + k, qual=lambda ql: rng.integers(0, 42, ql)))
    assert all(ref_end(r) <= GAP[0] or r["pos0"] >= GAP[1] for r in reads) and max(ref_end(r) for r in reads) <= 400
    return reads


def _region_rows(t):
    pile = region_pile()

    def row(name, begin, end, reads=pile):
        w = end - begin
        t.append(Row("region/" + name, "region", reads, REGION_REF, begin, end, 3, 0,
                     (dict(tiles=(w + TILE - 1) // TILE, last_tile=(w - 1) % TILE + 1),)))
    for b in REGION_BEGINS:
        for w in REGION_WIDTHS:
            row("b%d/w%d" % (b, w), b, b + w)
    row("no_read", GAP[0] + 3, GAP[1] - 3)
    row("past_last_read", 405, 470)
    last = read(len(REGION_REF) - 32, "32M", 3999)
    row("end_is_ref_len", len(REGION_REF) - 70, len(REGION_REF), pile + [last])
    row("reads_start_at_or_after_end", 0, 100)                      # tile 1 is positions 64 .. 99; reads start at 100, 101, 110


def boundary_table():
    t = []
    _row_rows(t)
    _round_rows(t)
    _region_rows(t)
    assert len({r.name for r in t}) == len(t)
    return t


_ORACLE = {}


def oracle_out(oracle, row):
    """orc_pileup_region (oracle/pyoracle.py) on a row, computed once for all the tests that compare with it"""
    if row.name not in _ORACLE:
        P = oracle.pack_reads(row.reads, row.ref.encode())
        _ORACLE[row.name] = oracle.pileup_region(P, row.begin, row.end, min_plp_bq=row.min_plp_bq, min_plp_idq=row.min_plp_idq,
                                                 use_baq=True)
    return _ORACLE[row.name]
