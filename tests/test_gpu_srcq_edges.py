"""-m gpu: the source-quality kernel at its routing boundaries (tests/srcq_edges.py), one test per table row: K on either side
of LFQ_SRCQ_LDS_CELLS (LDS or the scratch slice), of the 64 and 128 cells the lanes stride over, the pruning exit at its first
possible row and long before the last one, LDS and scratch reads in neighbouring wavefronts of one launch, and more reads than
the launch has wavefronts.  The integers equal those of oracle.source_qual, in the given and in reversed read order."""
import pytest

import srcq_edges as se

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TABLE = se.boundary_table()


def test_table_sits_on_the_boundaries():
    assert (se.LDS_CELLS, se.WAVES, se.STRIDE) == (768, 4, 64)
    assert se.K_SET == (1, 2, 62, 63, 64, 65, 127, 128, 129, 766, 767, 768, 769)
    assert [row.reads[0]["K"] for row in TABLE if row.kind == "K"] == list(se.K_SET)
    for row in TABLE:
        for r in row.reads:
            n, m = se.count(r)
            assert m - 1 == r["K"] and n >= m, r["name"]              # K by counting, as count_cigar_ops does
            assert r["K"] >= 1 or row.kind == "grid"                  # (the grid row has reads without a non-match between the others)
    for row in TABLE:
        if row.kind == "grid":
            continue
        for r in row.reads:
            (n, m), (left_at, rows) = se.count(r), se.exit_row(r)
            if "early" in r["name"] or r["name"][:2] in ("n2", "n3"):
                assert n > 2 * m and left_at < rows - r["K"], r["name"]       # the exit fires, long before the last row
            else:
                assert n == m == rows == left_at, r["name"]                   # ... cannot fire before the last row
    (nb,) = [row for row in TABLE if row.kind == "neighbours"]
    assert [r["K"] for r in nb.reads[:3]] == [se.LDS_CELLS - 1, se.LDS_CELLS, se.LDS_CELLS - 1]


@pytest.mark.parametrize("row", TABLE, ids=se.row_id)
def test_row(caller, oracle, row):
    import torch
    import lofreq_amd as la
    reads = row.reads
    if row.kind == "grid":          # the grid-stride loop runs, and with it the reset of a wavefront's histogram
        n_waves = se.WAVES * se.C["BLOCKS_PER_CU"] * torch.cuda.get_device_properties(0).multi_processor_count
        assert len(reads) > n_waves
    want = [oracle.source_qual(r["pos0"], r["cigar"], r["seq"], r["qual"], se.REF, nonmatch_qual=-1, min_bq=se.MIN_BQ) for r in reads]
    assert row.kind == "grid" or any(v > 0 for v in want)
    for rr, exp, what in ((reads, want, "as given"), (reads[::-1], want[::-1], "reversed")):
        sq, sqb = la.source_qual_batch(caller, rr, se.REF, def_nm_q=-1, min_bq=se.MIN_BQ)
        bad = [(what, r["name"], int(g), e) for r, g, e in zip(rr, sq, exp) if int(g) != e]
        assert not bad, (len(bad), bad[:8])
        assert [int(v) for v in sqb] == [min(max(e, 0), 254) for e in exp]
