"""CPU half of the viterbi boundary tests (tests/viterbi_edges.py): every read has the geometry its row claims and the table
covers the listed values; the Python model (tests/viterbi_model.py) reproduces the stored results and equals the reference's
2.1.4 binary on every read the binary can be asked about (tests/golden/viterbi_edges.json)."""
import pytest

import viterbi_edges as ve
import viterbi_model as vm

TABLE = ve.boundary_table()
FIX = ve.load_fixture()


def _reads(kind=None):
    return [(row, r, ve.geometry(r)) for row in TABLE for r in row.reads if kind is None or row.kind == kind]


def test_constants_are_the_kernels():
    assert (ve.RWIN, ve.STRIP, ve.PACK, ve.LOAD, ve.GATHER) == (10, 64, 4, 64, 64)


def test_every_read_has_the_geometry_it_claims():
    assert {row.kind for row in TABLE} == set(ve.KINDS)
    for row, r, g in _reads():
        assert g.n_strips == (g.q + 63) >> 6 and g.rows == min(64, g.q - ((g.n_strips - 1) << 6)) and g.n_steps == g.w + g.rows - 1
        assert 0 <= g.lower < g.upper <= len(ve.CONTIGS[row.contig]) and g.q >= 1, (row.name, r["name"])
        for k, v in r["claim"].items():
            assert getattr(g, k) == v, (row.name, r["name"], k, v, g)
        assert sum(l for op, l in r["cigar"] if op in "MIS=X") == len(r["seq"]) == len(r["qual"])


def test_covered_values():
    q_claimed = {r["claim"]["q"] for _, r, _ in _reads("q")}
    assert q_claimed == {1, 1030} | set(ve.Q_SET)
    assert {vm.cigar_str(r["cigar"]) for _, r, g in _reads("q") if g.q == 1} >= {"1I", "1M2D"}
    assert max(g.n_strips for _, _, g in _reads("q")) == 17
    for q in ve.Q_SET:              # the 2-base deletion the table is asked for, and a twin the binary can be asked about
        assert {r["name"] for _, r, g in _reads("q") if g.q == q} == {"q%d_2D" % q, "q%d_1D" % q}
    w_rows = _reads("w")
    tail = [(r, g) for _, r, g in w_rows if r["name"].startswith("tail_ins")]
    w_rows = [x for x in w_rows if not x[1]["name"].startswith("tail_ins")]
    assert {g.n_strips for _, g in tail} == {2, 3} and all(g.upper == ve.MAIN_LEN and r["cigar"][-1][0] == "I" for r, g in tail)
    assert {r["claim"]["w"] for _, r, _ in w_rows} == set(ve.W_SET)
    for w in ve.W_SET:              # two reads, one of them at least of two or more strips (the guarded hand-over load)
        assert len({g.n_strips for _, r, g in w_rows if g.w == w}) == 2 and any(g.n_strips > 1 for _, r, g in w_rows if g.w == w)
    steps = {g.n_steps for _, _, g in _reads("n_steps")}
    assert {n % ve.PACK for n in steps} == set(range(ve.PACK)) and {n % ve.LOAD for n in steps} >= {0, 1, ve.LOAD - 1}
    assert {g.n_strips for _, _, g in _reads("n_steps")} == {1, 2}
    short = [(r, g) for _, r, g in _reads("w<q")]
    assert all(g.w < g.q for _, g in short) and "10M100I10M" in {vm.cigar_str(r["cigar"]) for r, _ in short}
    assert any(g.q > 128 and g.w < 64 for _, g in short)
    long_ = [(r, g) for _, r, g in _reads("w>>q")]
    assert {vm.cigar_str(r["cigar"]) for r, _ in long_} >= {"40M%dD40M" % d for d in ve.LONG_DELS}
    assert any(g.q > 64 and g.w > 600 for _, g in long_)
    before = {}                     # rows directly in front of an I / a D
    for _, r, _ in _reads("strip edge"):
        y = 0
        for op, l in r["cigar"]:
            if op in "ID":
                before.setdefault(op, set()).add(y)
            y += l if op in "MI" else 0
    assert before["I"] >= set(ve.EDGE_ROWS) | {62} and before["D"] >= set(ve.EDGE_ROWS)
    clipped = _reads("clipped")
    assert {r["pos0"] for row, r, _ in clipped if row.contig == "main"} >= {0, 3, 9, 10, 11}
    assert {ve.MAIN_LEN - (r["pos0"] + 61) for row, r, g in clipped if row.contig == "main" and r["pos0"] > 100} == {0, 9, 10}
    assert any(g.lower == 0 and g.upper == ve.SHORT_LEN and r["pos0"] > 0 for row, r, g in clipped if row.contig == "short")


def test_tie_and_quality_rows():
    main = ve.CONTIGS["main"]
    assert main[ve.PA_AT:ve.PA_AT + ve.PA_LEN] == "A" * ve.PA_LEN and ve.PA_LEN >= 200
    assert main[ve.AT_AT:ve.AT_AT + 2 * ve.AT_UNITS] == "AT" * 40
    ties = _reads("tie")
    pa = [(r, g) for _, r, g in ties if r["name"].startswith("pa_")]
    for r, g in pa:                 # one letter over a window of the same letter, the read shorter than the window
        if r["name"].startswith("pa_last_ins"):
            assert r["seq"][-1] == "C" and r["qual"][-1] == 93 and set(r["seq"][:-1]) == {"A"} and r["cigar"][-1] == ("I", 1)
            continue
        assert set(r["seq"]) == {"A"} and set(main[g.lower:g.upper]) == {"A"} and g.q < g.w
    assert {tuple(sorted(set(r["qual"]))) for r, _ in pa} == {(30,), (2, 30), (30, 93)}
    assert all(sum(v != 2 for v in r["qual"]) == 1 for r, _ in pa if 2 in r["qual"])
    at = [r for _, r, _ in ties if r["name"].startswith("at_")]
    assert {r["cigar"][0][1] for r in at if r["cigar"][1][0] == "D"} == {20, 20 + ve.AT_UNITS, 18 + 2 * ve.AT_UNITS}
    assert all(set(r["qual"]) == {30} for r in at)
    (qrow,) = [row for row in TABLE if row.kind == "quality"]
    assert qrow.dqs == (-1, 0, 20, 93)
    by = {r["name"]: r for r in qrow.reads}
    assert sum(v != 2 for v in by["q2_but_one"]["qual"]) == 1
    rest = sorted(v for v in by["q2_even_median"]["qual"] if v != 2)
    assert len(rest) % 2 == 0 and (rest[len(rest) // 2] + rest[len(rest) // 2 - 1]) % 2 == 1
    assert {0, 93} <= set(by["q0_q93"]["qual"]) and 2 in by["q2_runs"]["qual"]
    ops = [(op, l) for _, r, _ in _reads("gather") for op, l in r["cigar"]]
    for op in "MIS":
        assert any(o == op and ve.GATHER < l <= 2 * ve.GATHER for o, l in ops) and any(o == op and l > 2 * ve.GATHER for o, l in ops)
    assert any([op for op, _ in r["cigar"]][:2] == ["S", "I"] for _, r, _ in _reads("gather"))


def test_fixture_holds_the_table():
    assert FIX["contigs"] == ve.CONTIGS and FIX["def_quals"] == list(ve.DEF_QUALS)
    assert [x["name"] for x in FIX["rows"]] == [row.name for row in TABLE]
    for row, x in zip(TABLE, FIX["rows"]):
        assert x["reads"] == [ve.inline_read(r) for r in row.reads] and x["contig"] == row.contig
        assert x["def_quals"] == list(row.dqs) and set(x["model"]) == set(x["binary"]) == {str(d) for d in row.dqs}


@pytest.mark.parametrize("row", TABLE, ids=ve.row_id)
def test_model_reproduces_the_fixture_and_equals_the_binary(row):
    x = FIX["rows"][TABLE.index(row)]
    for dq in row.dqs:
        for r, m, b in zip(row.reads, x["model"][str(dq)], x["binary"][str(dq)]):
            assert ve.model_result(r, dq) == m, (r["name"], dq)
            # the binary is left out exactly where it cannot be asked
            assert (b is not None) == ve.in_binary_domain(r, m), (r["name"], dq)
            assert b is None or b == m[:2], (r["name"], dq, m, b)


def test_rows_outside_the_binarys_domain():
    """which they are: every single deletion of two or more bases (d - 1 bytes past ref[]), nothing else"""
    outside = set()
    for row, x in zip(TABLE, FIX["rows"]):
        for r, b in zip(row.reads, x["binary"][str(row.dqs[0])]):
            if b is None:
                outside.add(r["name"])
                dels = [l for op, l in r["cigar"] if op == "D"]
                assert len(dels) == 1 and dels[0] >= 2, r["name"]
    assert {"q1_1M2D", "del100", "del300", "del400", "del600", "del600_q100", "pa_del2", "at_del_left"} <= outside
    assert sum(len(row.reads) for row in TABLE) - len(outside) >= 80
