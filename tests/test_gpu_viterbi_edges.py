"""-m gpu: the viterbi kernels at their geometry boundaries (tests/viterbi_edges.py), one test per table row.  Position, CIGAR
and status of every read are compared for equality with the results stored in tests/golden/viterbi_edges.json -- the Python
model's, which tests/test_viterbi_edges.py holds to the 2.1.4 binary wherever the binary can be asked -- with every -q of the
row, on four roads: lfq_viterbi_batch on the row alone, the row behind four plain realigned reads (another place in the
workgroup, other offsets into the back pointers and the hand-over rows), the row reversed, and the row (sorted by position, as
a read set has to be) through lfq_readset_viterbi, where lfq_vit_gather_kernel builds query, -q stand-in and window."""
import numpy as np
import pytest

import viterbi_edges as ve
import viterbi_model as vm

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TABLE = ve.boundary_table()
FIX = ve.load_fixture()
OPS = "MIDNSHP=X"


def _stored(row, dq):
    x = FIX["rows"][TABLE.index(row)]
    assert x["name"] == row.name and x["reads"] == [ve.inline_read(r) for r in row.reads]
    return [tuple(m) for m in x["model"][str(dq)]]


def _batch(caller, reads, contig, dq):
    from lofreq_amd import viterbi as lv
    got = lv.viterbi_batch(caller, [ve.lib_read(r) for r in reads], ve.CONTIGS[contig].encode(), dq)
    return [(p, vm.cigar_str(c), s) for p, c, s in got]


def _resident(caller, reads, contig, dq):
    """the reads, which are sorted by position, through ReadSet.viterbi -> results in the order of `reads`"""
    import lofreq_amd as la
    from test_gpu_readset_viterbi import flat
    rs = la.ReadSet.from_arrays(caller, flat(reads, ve.CONTIGS[contig]))
    new, (pos, status, cig_off, cig), order = rs.viterbi(dq)
    new.close()
    rs.close()
    assert sorted(order) == list(range(len(reads)))
    return [(int(pos[i]), "".join("%d%s" % (int(w) >> 4, OPS[int(w) & 15]) for w in cig[cig_off[i]:cig_off[i + 1]]), int(status[i]))
            for i in range(len(reads))]


@pytest.mark.parametrize("row", TABLE, ids=ve.row_id)
def test_row(caller, row):
    pad = ve.pad_reads(TABLE, row.contig)
    names = [r["name"] for r in row.reads]
    for dq in row.dqs:
        want = _stored(row, dq)
        want_pad = _stored([x for x in TABLE if x.kind == "pad" and x.contig == row.contig][0], dq if dq in (-1, 20) else -1)
        assert _batch(caller, row.reads, row.contig, dq) == want, ("alone", dq, names)
        assert _batch(caller, pad + row.reads, row.contig, dq) == want_pad + want, ("behind four reads", dq, names)
        assert _batch(caller, row.reads[::-1], row.contig, dq) == want[::-1], ("reversed", dq, names)
        by_pos = sorted(range(len(row.reads)), key=lambda i: row.reads[i]["pos0"])
        got = _resident(caller, [row.reads[i] for i in by_pos], row.contig, dq)
        assert got == [want[i] for i in by_pos], ("resident", dq, [names[i] for i in by_pos])
