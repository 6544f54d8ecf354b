"""CPU half of the pileup tile boundary tests (tests/pileup_edges.py): the two resolvers of lfq_pileup.hip restated and held
against every row's claims, the table against the list of boundaries it must have a row on each side of, a numpy model of the
SNV tile kernel's fast path against the oracle -- and two wrong variants of it against the rows meant to catch them -- and the
two references of the indel fields against each other."""
import numpy as np
import pytest

import golden_util as gu
import pileup_edges as pe

TABLE = pe.boundary_table()
BY_NAME = {r.name: r for r in TABLE}
ROWS = [r for r in TABLE if r.group == "row"]
OPS = pe.OPS
M_OPS, D_OPS = (0, 7, 8), (2, 3)


def _cg(read):
    return [(OPS.index(o), l) for o, l in read["cigar"]]


# ---- lfq_tile_resolve / lfq_tile_resolve_indel, restated --------------------------------------------------------------------

def _stretches(cg, x, p0, tile, stop_at_tile_end):
    """the walk both resolvers share: the masks, the stretches (q, dp, n) joined as the kernels join them, and the count"""
    cm = dm = 0
    y = nseg = 0
    s1 = s2 = None
    d_slow = False
    events = []
    for k, (op, l) in enumerate(cg):
        if stop_at_tile_end and not x < p0 + tile:
            break
        if op in M_OPS or op in D_OPS:
            a, b = max(x, p0), min(x + l, p0 + tile)
            if a < b:
                n, sh = b - a, a - p0
                mk = ((1 << n) - 1) << sh
                if op in D_OPS:
                    dm |= mk
                    opn = cg[k + 1][0] if k + 1 < len(cg) else -1
                    if opn not in M_OPS or x + l >= p0 + tile:
                        d_slow = True
                else:
                    q = y + (a - x)
                    cm |= mk
                    if nseg == 0:
                        s1, nseg = [q, sh, n], 1
                    elif nseg == 1 and q == s1[0] + s1[2] and sh == s1[1] + s1[2]:
                        s1[2] += n
                    elif nseg == 1:
                        s2, nseg = [q, sh, n], 2
                    elif nseg == 2 and q == s2[0] + s2[2] and sh == s2[1] + s2[2]:
                        s2[2] += n
                    else:
                        nseg += 1
            pl = x + l - 1
            if l > 0 and p0 <= pl < p0 + tile:
                v = _peek(cg, k)
                if v:
                    events.append((pl - p0, v))
            x += l
            if op in M_OPS:
                y += l
        elif op in (1, 4):
            y += l
    return dict(cm=cm, dm=dm, nseg=nseg, s1=s1, s2=s2, d_slow=d_slow, events=events, end=x)


def _peek(cg, k):
    """resolve_cigar2's look at what follows operation k"""
    if k + 1 >= len(cg):
        return 0
    op2, l2 = cg[k + 1]
    if op2 == 2:
        return -l2
    if op2 == 1:
        return l2
    if op2 == 6 and k + 2 < len(cg):
        l3 = 0
        for o3, ll in cg[k + 2:]:
            if o3 == 1:
                l3 += ll
            elif o3 in (2, 0, 3, 7, 8):
                break
        return l3
    return 0


def _row_geometry(W, s0, words):
    out = dict(a0=0, nw=0, off0=0, off1=0, split=64, a=None)
    if W["nseg"] in (1, 2):
        q1, p1, n1 = W["s1"]
        g0 = s0 + q1
        a0 = g0 & ~15
        if W["nseg"] == 1:
            span = n1
        else:
            q2, p2, n2 = W["s2"]
            span = q2 + n2 - q1
        nw = ((g0 - a0) + span + 15) >> 4
        off0 = (g0 - a0) - p1
        off1 = off0 if W["nseg"] == 1 else (g0 - a0) + (q2 - q1) - p2
        out = dict(a0=a0, nw=nw, off0=off0, off1=off1, split=64 if W["nseg"] == 1 else p2, a=g0 - a0)
    out["over"] = W["nseg"] > 2 or out["nw"] > words
    return out


def tile_resolve(cigar, pos, s0, p0, tile, words=pe.WORDS):
    """lfq_tile_resolve; `words`: the word count its capacity test accepts (the kernel's: what the row holds)"""
    W = _stretches(cigar, pos, p0, tile, True)
    G = _row_geometry(W, s0, words)
    if G["over"]:
        G.update(nw=0, off0=0, off1=0, split=64)
    return dict(cm=W["cm"], dm=W["dm"], nseg=W["nseg"], slow=G["over"], **{k: G[k] for k in ("a0", "nw", "off0", "off1", "split", "a")})


def tile_resolve_indel(cigar, pos, s0, p0, tile):
    """lfq_tile_resolve_indel"""
    W = _stretches(cigar, pos, p0, tile, False)
    G = _row_geometry(W, s0, pe.WORDS)
    nev = len(W["events"])
    slow = W["d_slow"] or G["over"] or nev > pe.EV_CAP or (W["nseg"] == 0 and W["dm"] != 0)
    e = W["end"] - 1
    tail = e - p0 if p0 <= e < p0 + tile and (W["cm"] >> (e - p0)) & 1 else pe.NO_TAIL
    return dict(cm=W["cm"], dm=W["dm"], nseg=W["nseg"], slow=slow, nev=nev, events=W["events"][:pe.EV_CAP], tail_dp=tail,
                nw=0 if slow else G["nw"], off0=G["off0"], off1=G["off1"], split=G["split"], a0=G["a0"])


def _tile_of(row, k):
    c0 = k * pe.TILE
    return row.begin + c0, min(pe.TILE, row.end - row.begin - c0)


def classes(row, c):
    """the class of the claim's read in the claim's tile, by the restated resolvers, in the claim's own terms"""
    r = row.reads[c["read"]]
    s0 = int(pe.seq_offsets(row.reads)[c["read"]])
    p0, tile = _tile_of(row, c["tile"])
    S = tile_resolve(_cg(r), r["pos0"], s0, p0, tile)
    I = tile_resolve_indel(_cg(r), r["pos0"], s0, p0, tile)
    got = dict(read=c["read"], tile=c["tile"], a=S["a"], nseg=S["nseg"], nw=S["nw"], slow=S["slow"], slow_indel=I["slow"],
               nev=I["nev"], tail_dp=I["tail_dp"])
    if "off1_neg" in c:
        got["off1_neg"] = S["off1"] < 0
    return got


# ---- the table --------------------------------------------------------------------------------------------------------------

def test_rows_are_small_and_sorted():
    counts = {}
    for r in TABLE:
        counts[r.group] = counts.get(r.group, 0) + 1
        pos = [x["pos0"] for x in r.reads]
        assert pos == sorted(pos), r.name
        assert len(r.ref) <= 1024 and len(r.reads) <= 600, r.name
        assert 0 <= r.begin < r.end <= len(r.ref) and all(pe.ref_end(x) <= len(r.ref) for x in r.reads), r.name
        lb = [x["lb"] is None for x in r.reads]
        assert all(lb) or not any(lb), r.name             # a read set has the lb tag for every read or for none
    print("rows per group:", counts)
    assert set(counts) == {"row", "round", "region"}


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_marked_read_has_the_class_the_row_claims(name):
    row = BY_NAME[name]
    assert row.claim and row.reads[row.claim[0]["read"]].get("mark")
    for c in row.claim:
        assert classes(row, c) == c, name


def _claims():
    return [(r, c) for r in ROWS for c in r.claim]


# every boundary of the issue: name -> (what a claim on one side looks like, ... on the other side)
def _boundaries():
    whole_ins = lambda c, a, fast: c["a"] == a and c["nseg"] == 2 and (c["nw"] == pe.WORDS if fast else c["slow"])
    B = {}
    for a in pe.ALIGNMENTS:
        B["insertion capacity, a = %d" % a] = (lambda r, c, a=a: "ins_capacity" in r.name and whole_ins(c, a, True),
                                               lambda r, c, a=a: "ins_capacity" in r.name and whole_ins(c, a, False))
        B["one stretch of a tile, a = %d" % a] = (lambda r, c, a=a: c["a"] == a and c["nseg"] == 1 and c["nw"] == (a + pe.TILE + 15) // 16
                                                  and "one_stretch" in r.name,
                                                  lambda r, c, a=a: c["a"] == a and c["nseg"] == 1 and c["nw"] == 1)
    B["stretches: one | two"] = (lambda r, c: "join/eq_X_M" in r.name and c["nseg"] == 1,
                                 lambda r, c: "join/eq_I_X_M" in r.name and c["nseg"] == 2)
    B["stretches: two | three"] = (lambda r, c: "a_tile_apart" in r.name and c["nseg"] == 2 and not c["slow"],
                                   lambda r, c: "one_tile" in r.name and c["nseg"] == 3 and c["slow"])
    B["second offset negative"] = (lambda r, c: c.get("off1_neg") is True and c["nw"] == 1,
                                   lambda r, c: c.get("off1_neg") is True and c["nw"] >= 4)
    B["insertion at the tile edge: after the last dp | before dp 0"] = (
        lambda r, c: "ins_after" in r.name and c["tile"] == pe.MT and c["nev"] == 1 and c["nseg"] == 1,
        lambda r, c: "ins_after" in r.name and c["tile"] == pe.MT + 1 and c["nev"] == 0 and c["nseg"] == 1)
    B["deletion against the tile end"] = (lambda r, c: "del_then_M" in r.name and c["tile"] == pe.MT and not c["slow_indel"],
                                          lambda r, c: "del_reaches" in r.name and c["tile"] == pe.MT and c["slow_indel"] and not c["slow"])
    B["deletion from the previous tile"] = (lambda r, c: "ends_dp0" in r.name and c["tile"] == pe.MT and not c["slow_indel"],
                                            lambda r, c: "ends_dp5" in r.name and c["tile"] == pe.MT and not c["slow_indel"])
    B["tile inside a deletion | a skip"] = (lambda r, c: "inside_D" in r.name and c["nseg"] == 0 and c["slow_indel"] and not c["slow"],
                                            lambda r, c: "inside_N" in r.name and c["nseg"] == 0 and c["slow_indel"] and not c["slow"])
    B["after a deletion: a match | anything else"] = (
        lambda r, c: r.name == "row/deletion/dlen1" and not c["slow_indel"],
        lambda r, c: "after_del/D_" in r.name and c["slow_indel"] and not c["slow"])
    for what in ("D_I", "D_N", "D_S", "D_last"):
        B["after a deletion: " + what] = (lambda r, c, what=what: what in r.name and c["slow_indel"], lambda r, c: "M_P_I_M" in r.name and not c["slow_indel"])
    B["clips: leading | trailing"] = (lambda r, c: "clip/leading" in r.name, lambda r, c: "clip/trailing" in r.name)
    B["event cap"] = (lambda r, c: c["nev"] == pe.EV_CAP, lambda r, c: c["nev"] == pe.EV_CAP + 1 and c["slow_indel"])
    B["third event at the last dp"] = (lambda r, c: c["nev"] == pe.EV_CAP and "last_at_dp" in r.name, lambda r, c: c["nev"] == pe.EV_CAP and c["tail_dp"] != pe.NO_TAIL)
    B["tail at dp 0 | at the last dp"] = (lambda r, c: c["tail_dp"] == 0, lambda r, c: c["tail_dp"] == pe.TILE - 1)
    B["tail: last M then I | then S"] = (lambda r, c: "M_then_I" in r.name and c["tail_dp"] == 29, lambda r, c: "M_then_S" in r.name and c["tail_dp"] == 29)
    B["tail: a covered position | a deleted one"] = (lambda r, c: "tail/M_then_S" in r.name and c["tail_dp"] != pe.NO_TAIL,
                                                     lambda r, c: "ends_in_D" in r.name and c["tail_dp"] == pe.NO_TAIL)
    return B


def test_table_has_a_row_on_each_side_of_every_boundary():
    claims = _claims()
    for name, sides in _boundaries().items():
        for i, side in enumerate(sides):
            assert any(side(r, c) for r, c in claims), (name, "side %d" % i)
    # the gates and the bytes: the values on both sides are in the marked read
    mark = lambda n: next(x for x in BY_NAME[n].reads if x.get("mark"))
    r = BY_NAME["row/bytes/bq_gate"]
    assert {r.min_plp_bq - 1, r.min_plp_bq} == set(mark(r.name)["qual"].tolist())
    assert {93, 94, 255} <= set(mark("row/bytes/bq_cap")["qual"].tolist())
    assert {32, 33, 126} <= set(mark("row/bytes/lb")["lb"].tolist())
    assert all(x["lb"] is None for x in BY_NAME["row/bytes/no_lb"].reads)
    assert set(range(4, 16)) <= set(mark("row/bytes/base_codes")["seq"].tolist())
    r = BY_NAME["row/bytes/idq_gate"]
    for k in ("bi", "bd"):
        assert {33 + r.min_plp_idq - 1, 33 + r.min_plp_idq} == set(mark(r.name)[k].tolist())
    assert {(x["bi"] is None, x["bd"] is None) for x in r.reads} == {(False, False), (True, False), (False, True), (True, True)}


def _window(row, k):
    """[lo, hi) of tile k as the kernels search it: first read whose running maximum of ends exceeds p0, first read that starts
    behind the tile"""
    p0, tile = _tile_of(row, k)
    pmax = np.maximum.accumulate([pe.ref_end(r) for r in row.reads])
    pos = np.array([r["pos0"] for r in row.reads])
    lo = int(np.searchsorted(pmax, p0, side="right"))
    return lo, max(lo, int(np.searchsorted(pos, p0 + tile - 1, side="right")))


def test_round_rows_fill_the_windows_they_claim():
    sizes = set()
    for row in TABLE:
        if row.group != "round":
            continue
        (c,) = row.claim
        lo, hi = _window(row, c["tile"])
        assert hi - lo == c["window"], row.name
        sizes.add(c["window"])
        p0, tile = _tile_of(row, c["tile"])
        over = np.array([r["pos0"] < p0 + tile and pe.ref_end(r) > p0 for r in row.reads[lo:hi]])
        if "empty" in c:
            n = pe.SLICE if c["empty"] == "slice" else pe.R
            blocks = over[: len(over) // n * n].reshape(-1, n)
            assert over[0] and (~blocks.any(1)).any() and over[-1], row.name        # a whole slice / round without overlap
        else:
            assert over.all(), row.name
        key = [(r["mapq"], int(r["qual"].max())) for r in row.reads if r["pos0"] == p0 - 8]
        assert len(set(key)) == len(key), row.name
    for rc in (pe.RC_COUNT, pe.RC_SCATTER, pe.RC_INDEL, pe.SLICE):
        assert {rc - 1, rc, rc + 1} <= sizes, rc


def test_region_rows_cover_the_tile_edges():
    rows = [r for r in TABLE if r.group == "region"]
    assert {(r.begin, r.end - r.begin) for r in rows} >= {(b, w) for b in pe.REGION_BEGINS for w in pe.REGION_WIDTHS}
    for r in rows:
        (c,) = r.claim
        w = r.end - r.begin
        assert c["tiles"] == -(-w // pe.TILE) and c["last_tile"] == w - (c["tiles"] - 1) * pe.TILE, r.name
    covered = lambda r, p: any(x["pos0"] <= p < pe.ref_end(x) for x in r.reads)
    r = BY_NAME["region/no_read"]
    assert not any(covered(r, p) for p in range(r.begin, r.end))
    assert any(pe.ref_end(x) <= r.begin for x in r.reads) and any(x["pos0"] >= r.end for x in r.reads)
    r = BY_NAME["region/past_last_read"]
    assert r.begin >= max(pe.ref_end(x) for x in r.reads)
    r = BY_NAME["region/end_is_ref_len"]
    assert r.end == len(r.ref) and pe.ref_end(r.reads[-1]) == len(r.ref)
    r = BY_NAME["region/reads_start_at_or_after_end"]
    last_tile_span = range(r.end, r.begin + r.claim[0]["tiles"] * pe.TILE)
    assert r.end in [x["pos0"] for x in r.reads] and sum(x["pos0"] in last_tile_span for x in r.reads) >= 3
    assert any(x["pos0"] < rr.begin < pe.ref_end(x) for rr in rows for x in rr.reads if rr.begin)      # reads that start before begin


# ---- the references --------------------------------------------------------------------------------------------------------------

oracle_out = pe.oracle_out


def _flat_keys(flat, sd, c):
    e0, e1 = int(flat["ev_off"][sd][c]), int(flat["ev_off"][sd][c + 1])
    ko, kc = flat["key_off"][sd], flat["key_chars"][sd]
    return [kc[int(ko[e]):int(ko[e + 1])].decode() for e in range(e0, e1)]


@pytest.mark.parametrize("group", ["row", "round", "region"])
def test_the_two_references_of_the_indel_fields_agree(oracle, group):
    """the oracle's column builder and golden_util.py_indel_pileup: coverage, tails, non-indels, ins, dels, non_fw / non_rv and
    the event keys of every column of every row"""
    n_ev = 0
    for row in TABLE:
        if row.group != group:
            continue
        out = oracle_out(oracle, row)
        flat = out["flat"]
        want = gu.py_indel_pileup(row.reads, row.ref, min_plp_idq=row.min_plp_idq)
        assert out["col_pos"].tolist() == sorted(p for p in want if row.begin <= p < row.end), row.name
        for c, p in enumerate(out["col_pos"].tolist()):
            w = want[p]
            got = tuple(int(flat[k][c]) for k in ("coverage_plp", "num_tails", "num_non_indels", "num_ins", "num_dels"))
            assert got == (w["cov"], w["tails"], w["non_indels"], w["n_ins"], w["n_dels"]), (row.name, p)
            for sd in range(2):
                assert (int(flat["non_fw"][sd][c]), int(flat["non_rv"][sd][c])) == (w["non_fw"][sd], w["non_rv"][sd]), (row.name, p, sd)
                keys = _flat_keys(flat, sd, c)
                assert keys == list(w["ev"][sd].keys()), (row.name, p, sd)
                n_ev += len(keys)
    assert n_ev > 0


def test_packed_layout_residues_of_the_observation_count(oracle):
    """the packed nt layout holds 8 observations a word: tables whose observation counts are 0, 1 and 7 mod 8 are in here"""
    seen = {int(oracle_out(oracle, r)["host"]["col_off"][-1]) % 8 for r in TABLE}
    assert {0, 1, 7} <= seen, seen


# ---- a numpy model of the SNV tile kernel ------------------------------------------------------------------------------------

def _locate(cg, x, p):
    y = 0
    for op, l in cg:
        if op in M_OPS:
            if p < x + l:
                return (1, y + p - x) if p >= x else (0, 0)
            x += l
            y += l
        elif op in D_OPS:
            if p < x + l:
                return (2 if p >= x else 0), 0
            x += l
        elif op in (1, 4):
            y += l
    return 0, 0


def model_tracks(row, words=pe.WORDS, second_offset=True, only=None):
    """lfq_pileup_tiles_kernel, both passes: per tile and read the resolver, the row of WORDS aligned words per track (a word
    past the stretch repeats its last one; what lies behind the row reads as 0 here), the bytes at off0 / off1 + dp; a slow read
    position by position.  words: what the capacity test accepts; second_offset=False: off0 behind `split` too; only: the one
    read these two changes apply to (None: every read)"""
    reads = row.reads
    so = pe.seq_offsets(reads)
    pad = np.zeros(32, np.uint8)
    cat = lambda k: np.concatenate([r[k] for r in reads] + [pad])
    qual, seq = cat("qual"), cat("seq")
    lb = cat("lb") if reads[0]["lb"] is not None else None
    cols = []
    for c0 in range(0, row.end - row.begin, pe.TILE):
        p0, tile = row.begin + c0, min(pe.TILE, row.end - row.begin - c0)
        obs = [[] for _ in range(tile)]
        cov = [0] * tile
        for i, r in enumerate(reads):
            cg = _cg(r)
            changed = only is None or i == only
            R = tile_resolve(cg, r["pos0"], int(so[i]), p0, tile, words if changed else pe.WORDS)
            rows = {}
            if R["nw"] > 0:
                for k, arr in (("q", qual), ("s", seq), ("b", lb)):
                    if arr is not None:
                        w = np.zeros(pe.ROW + 64, np.uint8)
                        for j in range(pe.WORDS):
                            o = R["a0"] + 16 * min(j, R["nw"] - 1)
                            w[16 * j:16 * j + 16] = arr[o:o + 16]
                        rows[k] = w
            for dp in range(tile):
                if (R["dm"] >> dp) & 1:
                    cov[dp] += 1
                if not (R["cm"] >> dp) & 1:
                    continue
                cov[dp] += 1
                if R["slow"]:
                    kind, qpos = _locate(cg, r["pos0"], p0 + dp)
                    assert kind == 1
                    g = int(so[i]) + qpos
                    bq, code, b = int(qual[g]), int(seq[g]), (int(lb[g]) if lb is not None else 0)
                else:
                    idx = (R["off0"] if dp < R["split"] or (changed and not second_offset) else R["off1"]) + dp
                    bq, code, b = int(rows["q"][idx]), int(rows["s"][idx]), (int(rows["b"][idx]) if lb is not None else 0)
                if bq >= row.min_plp_bq:
                    obs[dp].append((min(code, 4) | (8 if r["reverse"] else 0), min(bq, 93),
                                    (b - 33 if b >= 33 else 255) if lb is not None else 255, r["mapq"]))
        cols += [(p0 + dp, cov[dp], obs[dp]) for dp in range(tile) if cov[dp]]
    flat = [o for _, _, ob in cols for o in ob]
    tr = np.array(flat, np.int64).reshape(-1, 4).astype(np.uint8)
    off = np.zeros(len(cols) + 1, np.uint64)
    off[1:] = np.cumsum([len(ob) for _, _, ob in cols])
    return dict(col_pos=np.array([p for p, _, _ in cols], np.int64), col_off=off, coverage_plp=np.array([c for _, c, _ in cols], np.int32),
                num_bases=np.diff(off.astype(np.int64)).astype(np.int32), nt=tr[:, 0], bq=tr[:, 1], baq=tr[:, 2], mq=tr[:, 3])


def _equals_oracle(m, out):
    h = out["host"]
    n = int(h["col_off"][-1])
    return (np.array_equal(m["col_pos"], out["col_pos"]) and np.array_equal(m["col_off"], h["col_off"])
            and np.array_equal(m["coverage_plp"], h["coverage_plp"]) and np.array_equal(m["num_bases"], h["num_bases"])
            and all(np.array_equal(m[k], h[k][:n]) for k in ("nt", "bq", "baq", "mq")))


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_model_of_the_tile_kernel_gives_the_oracles_bytes(oracle, name):
    row = BY_NAME[name]
    assert _equals_oracle(model_tracks(row), oracle_out(oracle, row))


def test_rows_catch_a_capacity_test_off_by_one_word(oracle):
    """a resolver that takes WORDS + 1 words for fast while the row holds WORDS: wrong on every first-slow insertion row, and
    on no row whose marked read is fast"""
    hit = []
    for row in ROWS:
        wrong = not _equals_oracle(model_tracks(row, words=pe.WORDS + 1, only=row.claim[0]["read"]), oracle_out(oracle, row))
        if "ins_capacity" in row.name and row.claim[0]["slow"]:
            assert wrong, row.name
            hit.append(row.name)
        elif not any(c["slow"] for c in row.claim):
            assert not wrong, row.name
    assert len(hit) == len(pe.ALIGNMENTS)


def test_rows_catch_the_first_offset_used_for_the_second_stretch(oracle):
    """off0 behind `split`, for the marked read alone: wrong on every row where that read has two stretches in a tile on the
    fast path, and on no row where it has one everywhere"""
    hit = 0
    for row in ROWS:
        wrong = not _equals_oracle(model_tracks(row, second_offset=False, only=row.claim[0]["read"]), oracle_out(oracle, row))
        if any(c["nseg"] == 2 and not c["slow"] for c in row.claim):
            assert wrong, row.name
            hit += 1
        elif all(c["nseg"] <= 1 for c in row.claim):
            assert not wrong, row.name
    assert hit >= 10


# ---- a model of the indel tile kernel's counter pass ---------------------------------------------------------------------------

def _locate_indel(cg, x, p, l_qseq):
    """lfq_plp_locate_indel -> (kind, qpos, indel, tail)"""
    y = kind = qpos = indel = 0
    for k, (op, l) in enumerate(cg):
        m, d = op in M_OPS, op in D_OPS
        if (m or d) and kind == 0 and x <= p < x + l:
            kind = 1 if m else 2
            qpos = min(y + (p - x) if m else y, l_qseq - 1)
            if p == x + l - 1:
                indel = _peek(cg, k)
        if m or d:
            x += l
        if m or op in (1, 4):
            y += l
    return kind, qpos, indel, p == x - 1


def model_indel_counts(row):
    """lfq_plp_indel_tiles_kernel: {position: [cov, tails, non_indels, n_ins, n_dels, non_ins_fw, non_del_fw, sum of the insertion
    qualities of the entries without an insertion, ... deletion ... deletion, entries without an insertion, ... deletion]}"""
    reads = row.reads
    so = pe.seq_offsets(reads)
    pad = np.full(32, 33, np.uint8)
    tags = {k: np.concatenate([(r[k] if r[k] is not None else np.full(len(r["seq"]), 33, np.uint8)) for r in reads] + [pad])
            for k in ("bi", "bd")}
    out = {}
    for c0 in range(0, row.end - row.begin, pe.TILE):
        p0, tile = row.begin + c0, min(pe.TILE, row.end - row.begin - c0)
        for i, r in enumerate(reads):
            cg, s0 = _cg(r), int(so[i])
            R = tile_resolve_indel(cg, r["pos0"], s0, p0, tile)
            rows = {}
            if R["nw"] > 0:
                for k in ("bi", "bd"):
                    w = np.zeros(pe.ROW, np.uint8)
                    for j in range(pe.WORDS):
                        o = R["a0"] + 16 * min(j, R["nw"] - 1)
                        w[16 * j:16 * j + 16] = tags[k][o:o + 16]
                    rows[k] = w
            for dp in range(tile):
                covered, any_ = (R["cm"] >> dp) & 1, ((R["cm"] | R["dm"]) >> dp) & 1
                if not any_:
                    continue
                if not R["slow"]:
                    rest = R["cm"] >> dp
                    assert rest, (row.name, i, dp)              # a deleted position of a fast read has a covered one behind it
                    dpn = dp + ((rest & -rest).bit_length() - 1)
                    idx = (R["off0"] if dpn < R["split"] else R["off1"]) + dpn
                    assert 0 <= idx < pe.CAP, (row.name, i, dp)
                    iq = int(rows["bi"][idx]) - 33 if r["bi"] is not None else 0
                    dq = int(rows["bd"][idx]) - 33 if r["bd"] is not None else 0
                    indel = dict(R["events"]).get(dp, 0)
                    tail = bool(covered) and dp == R["tail_dp"]
                else:
                    kind, qpos, indel, tl = _locate_indel(cg, r["pos0"], p0 + dp, len(r["seq"]))
                    assert kind == (1 if covered else 2)
                    tail = kind == 1 and tl
                    iq = int(tags["bi"][s0 + qpos]) - 33 if r["bi"] is not None else 0
                    dq = int(tags["bd"][s0 + qpos]) - 33 if r["bd"] is not None else 0
                ok = not (iq < row.min_plp_idq or dq < row.min_plp_idq)
                no_ins, no_del, fw = ok and indel <= 0, ok and indel >= 0, not r["reverse"]
                c = out.setdefault(p0 + dp, [0] * 11)
                for k, v in enumerate((1, tail, ok and indel == 0, ok and indel > 0, ok and indel < 0, no_ins and fw, no_del and fw,
                                       iq if no_ins else 0, dq if no_del else 0, no_ins, no_del)):
                    c[k] += int(v)
    return out


@pytest.mark.parametrize("group", ["row", "round", "region"])
def test_model_of_the_indel_tile_kernel_gives_the_references_counts(group):
    """what the counter pass counts is what the scatter pass, which resolves every entry on its own, will write: the number of
    entries without an insertion / a deletion per position, with the other counts and the quality sums, against py_indel_pileup"""
    for row in TABLE:
        if row.group != group:
            continue
        want = gu.py_indel_pileup(row.reads, row.ref, min_plp_idq=row.min_plp_idq)
        got = model_indel_counts(row)
        assert sorted(got) == sorted(p for p in want if row.begin <= p < row.end), row.name
        for p, g in got.items():
            w = want[p]
            assert g == [w["cov"], w["tails"], w["non_indels"], w["n_ins"], w["n_dels"], w["non_fw"][0], w["non_fw"][1],
                         sum(q for q, _ in w["ne"][0]), sum(q for q, _ in w["ne"][1]), len(w["ne"][0]), len(w["ne"][1])], (row.name, p)
