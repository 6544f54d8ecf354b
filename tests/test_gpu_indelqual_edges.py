"""-m gpu: the indelqual kernels at their geometry boundaries (tests/indelqual_edges.py), one test per table row.  The BI / BD
bytes are compared for equality with the strings of tests/indelqual_model.py (held to the 2.1.4 binary on the same reads by
tests/test_indelqual_edges.py) on three roads: lfq_indelqual_batch, a resident ReadSet (indelqual, then fetch_indelquals) and
the batch with the reads in reversed order -- another seq_off layout over the same table.  The same rows in uniform mode check
the chunk arithmetic of the fill kernel alone."""
import numpy as np
import pytest

import indelqual_edges as ie
import indelqual_model as im
import indelqual_reads as ir

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TABLE = ie.boundary_table()
OPS = "MIDNSHP=X"


def _lib_reads(reads):
    return [{"pos0": r["pos0"], "cigar": r["cigar"], "seq": np.zeros(r["l_qseq"], np.uint8), "qual": np.zeros(r["l_qseq"], np.uint8)}
            for r in reads]


def _arrays(reads, ref):
    n = len(reads)
    cig = [(l << 4) | OPS.index(op) for r in reads for op, l in r["cigar"]]
    nb = sum(r["l_qseq"] for r in reads)
    return {"n": n, "ref": ref, "pos": np.array([r["pos0"] for r in reads], np.int32),
            "cig_off": np.cumsum([0] + [len(r["cigar"]) for r in reads]).astype(np.int64), "cig": np.array(cig or [0], np.uint32),
            "seq_off": np.cumsum([0] + [r["l_qseq"] for r in reads]).astype(np.int64), "seq": np.zeros(nb + 1, np.uint8),
            "qual": np.full(nb + 1, 30, np.uint8), "mapq": np.full(n, 60, np.uint8), "rev": np.zeros(n, np.uint8)}


@pytest.mark.parametrize("row", TABLE, ids=ie.row_id)
def test_row(caller, row):
    import lofreq_amd as la
    ref = ie.CONTIGS[row.contig].encode()
    want = ie.model_strings(row)
    uni = [im.uniform_read(r["l_qseq"], *ir.mode_quals(ie.UNIFORM)) for r in row.reads]
    names = [r["name"] for r in row.reads]
    for reads, exp, exp_u, what in ((row.reads, want, uni, "batch"), (row.reads[::-1], want[::-1], uni[::-1], "reversed")):
        got = la.indelqual_batch(caller, _lib_reads(reads), ref, "dindel")
        for r, (bi, bd), e in zip(reads, got, exp):
            assert bi.decode("latin-1") == e and bd == bi, (what, r["name"])
        got = la.indelqual_batch(caller, _lib_reads(reads), ref, "uniform", *ir.mode_quals(ie.UNIFORM))
        assert [(a.decode("latin-1"), b.decode("latin-1")) for a, b in got] == exp_u, (what, names)
    flat = "".join(want).encode("latin-1")
    rs = la.ReadSet.from_arrays(caller, _arrays(row.reads, ref))
    rs.indelqual("dindel")
    bi, bd = rs.fetch_indelquals()
    assert bi.tobytes() == flat and bd.tobytes() == flat, ("resident", names)
    rs.indelqual("uniform", *ir.mode_quals(ie.UNIFORM))
    bi, bd = rs.fetch_indelquals()
    rs.close()
    assert bi.tobytes() == "".join(u[0] for u in uni).encode() and bd.tobytes() == "".join(u[1] for u in uni).encode()
