"""CPU tests: the edge table of plp_summary's header line (tests/plpsummary_edges.py) sits where it says -- every line written
down there is what the restatement (tests/plpsummary_ref.py, held to the reference's binary by test_plpsummary_ref.py) gives for
the row's reads, every branch has a row, and the rows have the properties their names claim."""
import maxdepth_model as mdm
import plpsummary_edges as E
import plpsummary_ref as ref

ROWS = E.table()


def _columns(r):
    keep = mdm.kept_reads(r.reads, r.max_depth) if r.max_depth is not None else None
    return ref.summarize(r.reads, r.ref, r.begin, r.end, r.min_plp_bq, r.min_plp_idq, keep)


def test_every_expected_line_comes_from_the_restatement():
    assert len({r.name for r in ROWS}) == len(ROWS) >= 25
    for r in ROWS:
        got = {c["pos0"]: ref.format_line(E.CHROM, c) for c in _columns(r)}
        assert got == r.expect, r.name
        assert all(a["pos0"] <= b["pos0"] for a, b in zip(r.reads, r.reads[1:])), r.name       # pileup order = file order


def test_every_branch_has_a_row():
    covered = {b for r in ROWS for b in r.branches}
    assert covered == set(E.BRANCHES)
    assert E.wave_rounds() == 64


def _by_name(name):
    return [r for r in ROWS if r.name == name][0]


def test_the_rows_are_what_their_names_say():
    W = E.wave_rounds()
    for n in (W - 1, W, W + 1, 2 * W, 2 * W + 1):
        c = {c["pos0"]: c for c in _columns(_by_name("window_%d" % n))}[20]
        assert c["coverage"] == n and sum(c["fw"]) + sum(c["rv"]) <= n
    c = {c["pos0"]: c for c in _columns(_by_name("only_d"))}
    assert c[13]["coverage"] == 1 and c[13]["cons"] == "A" and sum(c[13]["fw"]) + sum(c[13]["rv"]) == 0
    c = _columns(_by_name("below_bq"))[0]
    assert c["coverage"] == 3 and c["cons"] == "A" and sum(c["fw"]) + sum(c["rv"]) == 0 and c["heads"] == 3
    c = _columns(_by_name("q0_dbl_min"))[0]
    assert c["cons"] == "C" and c["base_counts"][1] == 2 * ref.DBL_MIN
    for name in ("cap_93_120", "cap_93_94", "exact_tie"):
        c = _columns(_by_name(name))[0]
        s = sorted(c["base_counts"])
        assert s[-1] == s[-2] > 0 and c["cons"] == "A", name
    c = _columns(_by_name("n_and_iupac"))
    assert c[0]["base_counts"][3] == c[0]["base_counts"][4] and c[0]["cons"] == "T" and c[0]["fw"][4] + c[0]["rv"][4] == 2
    assert c[1]["cons"] == "N"
    # the order-dependent pair: the same multiset of qualities on both nucleotides, sums one ulp apart
    a = _columns(_by_name("near_tie_c"))[0]
    assert a["base_counts"][0] == 2.488733333549255 and a["base_counts"][1] == 2.4887333335492556 and a["cons"] == "C"
    b = _columns(_by_name("near_tie_a"))[0]
    assert b["base_counts"][1] == 2.488733333549255 and b["base_counts"][0] == 2.4887333335492556 and b["cons"] == "A"
    c = _columns(_by_name("clear_winner"))[0]
    assert c["fw"][0] + c["rv"][0] == 10 and c["fw"][1] == 1 and c["cons"] == "A"
    cons = lambda name, p: {c["pos0"]: c["cons"] for c in _columns(_by_name(name))}[p]
    assert cons("ins_wins", 12) == "+A" and cons("idq_decides", 12) == "T" and cons("ins_equal", 12) == "T"
    assert cons("two_events_tie", 12) == "+C" and cons("ins_before_del", 12) == "+GG" and cons("del_wins", 12) == "-AG"
    assert [c["pos0"] for c in _columns(_by_name("region_cut"))] == [9, 10, 11, 12, 13]
    assert _columns(_by_name("empty_region")) == [] and _by_name("empty_region").expect == {}
    r = _by_name("max_depth_2")
    assert mdm.kept_reads(r.reads, 2).tolist() == [1, 1, 0, 0, 0] and _columns(r)[0]["coverage"] == 2
