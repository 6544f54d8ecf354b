"""CPU half of the indelqual boundary tests (tests/indelqual_edges.py): the planted runs sit on the lane, tile, halo and contig
edges the rows name, the read sets have the chunk layout they name, and the Python model (tests/indelqual_model.py) gives the
bytes `lofreq indelqual --dindel` of the 2.1.4 binary wrote for every read (tests/golden/indelqual_edges.json)."""
import pytest

import indelqual_edges as ie
import indelqual_model as im

TABLE = ie.boundary_table()
FIX = ie.load_fixture()


def _rows(kind):
    return [r for r in TABLE if r.kind == kind]


def _row(prefix):
    (row,) = [r for r in TABLE if r.name.startswith(prefix)]
    return row


def test_constants_are_the_kernels():
    assert (ie.TILE, ie.HALO, ie.SAT, ie.LANE, ie.CHUNK, ie.BLOCK) == (4096, 32, 19, 16, 16, 4096)


def test_contigs():
    assert sorted(len(g) % ie.LANE for g in ie.CONTIGS.values()) == [0, 1, ie.LANE - 1]
    for name, g in ie.CONTIGS.items():
        count, n = im.homopolymer_counts(g), len(g)
        assert 2 * ie.TILE + ie.SITES[name][-1]["tab_begin"] + ie.HALO < n < 3 * ie.TILE
        for site in ie.SITES[name]:
            assert site["tab_begin"] % ie.LANE == 0 and site["tab_begin"] > 0
            for e, kind, start, L in site["plants"]:
                assert count[start] == L and g[start - 1].upper() != g[start].upper(), (name, site, kind)
        for kind, start, L in ie.LANE_PLANTS[name]:
            assert count[start] == L and g[start - 1].upper() != g[start].upper(), (name, kind, start)
    ends = {name: (im.homopolymer_counts(g), len(g)) for name, g in ie.CONTIGS.items()}
    # a run ending on the last base, one ending one base before it, one of more than 19 that the contig's end cuts
    assert ends["c0"][0][ends["c0"][1] - 5] == 5
    assert ends["c1"][0][ends["c1"][1] - ie.SAT] == ie.SAT - 1 and ends["c1"][0][ends["c1"][1] - 1] == 1
    assert ends["c15"][0][ends["c15"][1] - 25] == 25 > ie.SAT


def test_tile_rows_put_the_runs_on_their_own_tile_edges():
    """the lowest read of a row sets tab_begin; the row's planted runs lie around the two tile edges that follow from it, the
    reads cover them, and over all rows every start, end and case is there at both edges"""
    seen = {1: set(), 2: set()}
    lo_mod, ends = set(), set()
    site_of = {(c, s["tab_begin"]): s for c in ie.SITES for s in ie.SITES[c]}
    for row in _rows("tile"):
        g, ref_len = ie.geometry(row), len(ie.CONTIGS[row.contig])
        site = site_of[(row.contig, g.tab_begin)]
        assert g.tab_begin > 0 and g.tab_end in (ref_len - 1, ref_len) and g.edges == [g.tab_begin + ie.TILE, g.tab_begin + 2 * ie.TILE]
        assert 0 < ref_len - g.edges[-1] < ie.TILE                      # a partial last tile
        lo_mod.add(g.lo % ie.LANE)
        covered = set()
        for r in row.reads:
            x = r["pos0"]
            for op, l in r["cigar"]:
                if op in "M=X":
                    covered |= set(range(x, x + l))
                x += l if op in "M=XD" else 0
        for e, kind, start, L in site["plants"]:
            edge = g.edges[e - 1]
            assert set(range(start - 2, start + L + 1)) <= covered, (row.name, kind)
            seen[e].add((kind, start - edge, L))
            letters = ie.CONTIGS[row.contig][start:start + L]
            if kind in ("lower", "mixed"):
                assert letters[edge - start].islower() and letters.upper() != letters and not letters.islower()
            if kind == "N":
                assert set(letters) == {"N"} and start < edge < start + L
        last = max(r["pos0"] + sum(l for op, l in r["cigar"] if op in "M=XD") for r in row.reads)
        ends.add(last - ref_len)
    want = set(ie.edge_plants())
    assert seen[1] == want and seen[2] == want
    assert {("start", off, L) for L in (1, 2, 17, 18, 19, 20, 25) for off in (-1, 0, 1)} <= want
    assert {("end", off - L + 1, L) for L in (2, 18, 19, 20) for off in (-1, 0)} <= want
    # a run of 18 and of 19 that the last lane of a tile sees wholly in the halo: it starts on the edge
    assert {("start", 0, ie.SAT - 1), ("start", 0, ie.SAT)} <= want and ie.SAT <= ie.HALO
    assert lo_mod == {0, 1, ie.LANE - 1} and ends == {0, -1, 6}


def test_lane_rows():
    want = set(ie.lane_plants())
    assert {("start", off, L) for L in (1, 2, 17, 18, 19, 20, 25) for off in (-1, 0)} <= want
    assert {("end", off - L + 1, L) for L in (2, 18, 19, 20) for off in (-1, 0)} <= want and ("lower", -4, 8) in want
    for row in _rows("lanes"):
        g = ie.geometry(row)
        assert g.tab_begin > 0 and g.edges == []
        got = set()
        for kind, start, L in ie.LANE_PLANTS[row.contig]:
            edge = (start + ie.LANE // 2) // ie.LANE * ie.LANE if kind == "start" else (start + L) // ie.LANE * ie.LANE
            if kind == "lower":
                edge = start + 4
                assert ie.CONTIGS[row.contig][edge - 1:edge + 1].islower()
            assert edge % ie.LANE == 0 and g.lo < start - 2 and start + L + 1 < g.hi
            got.add((kind, start - edge, L))
        assert got == want


def test_read_set_rows():
    row = _row("reads of 1 to 17")
    assert sorted({r["l_qseq"] for r in row.reads}) == list(range(1, 18))
    owners = {len(o) for o in ie.chunk_owners(row)}
    assert {3, 4} <= owners and max(owners) >= 5
    row = _row("zero-length reads first")
    lens = [r["l_qseq"] for r in row.reads]
    assert lens[0] == 0 and lens[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(lens[1:-1], lens[2:-1]))
    assert any(a > 0 and b == 0 and c > 0 for a, b, c in zip(lens, lens[1:], lens[2:]))
    row = _row("a chunk edge before")
    g = ie.geometry(row)
    where = {}
    for r, off in zip(row.reads, g.seq_off):
        y = off
        for op, l in r["cigar"]:
            if op in "ISD":
                edge = (y + ie.CHUNK - 1) // ie.CHUNK * ie.CHUNK       # the first chunk edge at or behind the operation's start
                where.setdefault(op, set()).add("before" if edge == y and op != "D" else "on" if edge == y else
                                                "inside" if edge < y + l else "after" if edge == y + l else "far")
            y += l if op in "MIS=X" else 0
    assert where["I"] >= {"before", "inside", "after"} and where["S"] >= {"before", "inside", "after"}
    d = sorted((off + sum(l for op, l in r["cigar"][:1])) % ie.CHUNK for r, off in zip(row.reads, g.seq_off) if r["name"].startswith("d_"))
    assert d == [0, 1, ie.CHUNK - 1]                                   # the byte behind the deletion: on, after and before the edge
    nb = sorted(ie.geometry(r).n_bases for r in _rows("n_bases"))
    assert {n % ie.CHUNK for n in nb} >= {0, 1, ie.CHUNK - 1} and {ie.BLOCK, ie.BLOCK + 1} <= set(nb)
    for r in TABLE:
        assert ie.geometry(r).tab_begin > 0, r.name


@pytest.mark.parametrize("row", TABLE, ids=ie.row_id)
def test_model_gives_the_binarys_bytes(row):
    x = FIX["rows"][TABLE.index(row)]
    assert x["name"] == row.name and x["reads"] == [ie.inline_read(r) for r in row.reads]
    assert FIX["contigs"][row.contig] == ie.CONTIGS[row.contig]
    for r, m, b in zip(row.reads, ie.model_strings(row), x["bi"]):
        assert len(m) == r["l_qseq"]
        assert (b is None) == (r["l_qseq"] == 0), r["name"]             # the binary is asked about every read with bases
        assert b is None or im.unrle(b) == m, (row.name, r["name"])


def test_every_letter_of_the_table_occurs():
    letters = set()
    for row in TABLE:
        letters |= set("".join(ie.model_strings(row)))
    assert letters >= {"!", "M", "L", "6", "7"}        # counts 1 .. 4, 17, 18 and the '!' of 19 and more
