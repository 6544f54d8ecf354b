"""CPU tests: the edge table of plp_summary's quality lines (tests/plpquals_edges.py) sits where it says -- on the constants of
lfq_plp_group_kernel as the source states them, every branch has a row, every expected value is the restatement's
(tests/plpquals_ref.py, held to the reference's binary by test_plpquals_ref.py), and the rows have the properties their names
claim."""
import numpy as np

import maxdepth_model as mdm
import plpquals_edges as E
import plpquals_ref as Q

ROWS = E.table()
TRACKS = {r.name: r for r in ROWS if isinstance(r, E.TrackRow)}
READS = {r.name: r for r in ROWS if isinstance(r, E.ReadRow)}


def test_every_branch_has_a_row_and_the_constants_are_the_kernels():
    assert len(TRACKS) + len(READS) == len(ROWS) >= 20
    assert {b for r in ROWS for b in r.branches} == set(E.BRANCHES)
    assert E.kernel_constants() == (64, 4)


def test_every_expected_value_comes_from_the_restatement():
    for r in TRACKS.values():
        exp = Q.group_tracks(r.nt, r.bq, r.baq, r.mq, r.sq, r.col_off, r.c0, r.c1)
        assert exp == r.expect, r.name
        assert [Q.format_grouped(*exp, i, r.flag) for i in range(r.c1 - r.c0)] == r.text, r.name
        # a permutation of each column, stable inside a group
        nt_off = exp[0]
        assert nt_off[0] == 0 and nt_off[-1] == int(r.col_off[r.c1]) - int(r.col_off[r.c0]) and sorted(nt_off) == nt_off
        for i, c in enumerate(range(r.c0, r.c1)):
            a, b = int(r.col_off[c]), int(r.col_off[c + 1])
            assert nt_off[5 * i] == a - int(r.col_off[r.c0]) and nt_off[5 * i + 5] == b - int(r.col_off[r.c0])
            assert sorted(exp[1][nt_off[5 * i]:nt_off[5 * i + 5]]) == sorted(r.bq[a:b].tolist())
    for r in READS.values():
        keep = mdm.kept_reads(r.reads, r.max_depth) if r.max_depth is not None else None
        assert Q.text(E.CHROM, r.reads, r.ref, r.begin, r.end, r.flag, r.min_plp_bq, r.min_plp_idq, keep) == r.expect, r.name
        assert all(a["pos0"] <= b["pos0"] for a, b in zip(r.reads, r.reads[1:])), r.name


def test_the_rows_are_what_their_names_say():
    W, G = E.kernel_constants()
    for d in (1, W - 1, W, W + 1, 2 * W, 2 * W + 1):
        r = TRACKS["depth_%d" % d]
        assert int(r.col_off[2]) - int(r.col_off[1]) == d and len(r.col_off) == 4
        if d >= 5:
            assert all(b > a for a, b in zip(r.expect[0][5:10], r.expect[0][6:11]))      # all five groups in the column
    r = TRACKS["depth_0"]
    assert np.diff(r.col_off.astype(np.int64)).tolist() == [5, 0, 0, 4, 0] and r.text[1] == r.text[2] == r.text[4] == ""
    r = TRACKS["five_groups"]
    n = int(r.col_off[1])
    assert n == W + 1
    codes = [int(x) & 7 for x in r.nt]
    starts = r.expect[0][:5]
    seen = [0] * 5
    for i, k in enumerate(codes):                 # the rank of every observation differs from its lane, in both rounds
        assert starts[k] + seen[k] != i % W, i
        seen[k] += 1
    assert all(s > 0 for s in seen)
    assert {int(x) & 7 for x in TRACKS["one_group"].nt} == {2} and TRACKS["one_group"].text[0].count("\n") == 3
    assert {int(x) & 7 for x in TRACKS["only_n"].nt} == {4} and TRACKS["only_n"].text[0].startswith("  N\tBQ =")
    r = TRACKS["iupac"]
    assert {int(x) & 7 for x in r.nt} == {0, 1, 4, 5, 6, 7}
    assert r.expect[0][5] - r.expect[0][4] == sum(1 for x in r.nt if int(x) & 7 >= 4)     # codes above 4 count as N
    assert [TRACKS["ncols_%d" % n].c1 for n in (1, G, G + 1)] == [1, G, G + 1]
    r = TRACKS["range_offset_3"]
    assert r.c0 == 1 and int(r.col_off[r.c0]) % 4 == 3 and r.c1 == 4 < len(r.col_off) - 1
    r = TRACKS["no_baq"]
    assert r.baq is None and r.expect[2] is None and not r.flag & Q.LFQ_USE_BAQ and "BAQ =\t -1 -1" in r.text[0]
    r = TRACKS["sq_baq_mq_missing"]
    txt = "".join(r.text)
    assert " 49314" in txt and "SQ =" in txt and 254 in r.sq and 255 in r.sq and 255 in r.baq and 255 in r.mq
    sq_vals = [int(v) for l in txt.split("\n") if "\tSQ =" in l for v in l.split("\t")[2].split()]
    baq_vals = [int(v) for l in txt.split("\n") if "\tBAQ =" in l for v in l.split("\t")[2].split()]
    mq_vals = [int(v) for l in txt.split("\n") if "\tMQ =" in l for v in l.split("\t")[2].split()]
    assert sq_vals.count(49314) == 4 and sq_vals.count(-1) == 3 and baq_vals.count(-1) == 3 and mq_vals.count(255) >= 2
    assert 254 not in sq_vals and 255 not in sq_vals and 255 not in baq_vals
    assert int(r.col_off[2]) - int(r.col_off[1]) > W                                      # the long column crosses a round

    r = READS["below_bq"]
    assert len(r.expect) == 1 and "BQ =" not in r.expect[0] and "  +0\tIDQ =\t 0 0 0\n" in r.expect[0]
    r = READS["max_depth_2"]
    assert mdm.kept_reads(r.reads, 2).tolist() == [1, 1, 0, 0, 0] and "  +0\tIDQ =\t 0 0\n" in r.expect[0]
    r = READS["two_ins_one_del"]
    col = [b for b in r.expect if b.startswith("edge\t13\t")][0]
    assert col.index("  +A\tIQ =") < col.index("  +CC\tIQ =") < col.index("  -0\tIDQ =") < col.index("  -AG\tIDQ =")
    assert "  +A\tIQ =\t 30 34\n" in col and "  +A\tAQ =\t -1 -1\n" in col and "  +A\tSQ =\t -1 -1\n" in col
    assert "  N\tBQ =" in "".join(r.expect)                                               # the R and the N of the reads
    quiet = [b for b in r.expect if "\tins:0\tdels:0\t" in b]
    assert quiet and all("IQ =" not in b and "  +0\tIDQ =\t " in b and "  -0\tMQ =\t " in b for b in quiet)
    r = READS["one_side"]
    col = [b for b in r.expect if b.startswith("edge\t13\t")][0]
    assert "  -AG\tIDQ =" in col and "IQ =" not in col and [b.split("\t")[1] for b in r.expect] == ["12", "13", "14"]
    col = [b for b in READS["tagged"].expect if b.startswith("edge\t13\t")][0]
    assert "  +A\tAQ =\t 2 12\n" in col and "BAQ =\t -1" not in col
