"""-m gpu: the BAQ / IDAQ kernels at their routing and geometry boundaries (tests/baq_edges.py), one test per table row.
Everything is compared for equality with the oracle (tests/test_baq_edges.py holds the oracle to the reference's object and to
the 2.1.4 binary on the same reads): lb through lfq_baq_batch, lb / ai / ad and the tag flags through lfq_baq_idaq_batch, the
same bytes through a resident ReadSet, and the same bytes again with the row's reads behind a wavefront of plain 100-base
reads and in reversed order -- a read that is wrong only when its wavefront's Lmax, interior range or N flag comes from a
neighbour shows there.

Past the caps of the indel table (LFQ_BAQ_MAX_INDELS indels, LFQ_BAQ_MAX_TERMS repeat cells per read) the rule of
include/lofreq_amd.h holds as it stands: an indel the table did not take keeps '~', every indel it took carries the oracle's
byte, lb and the tag flags are the oracle's, and the other reads of the wavefront are untouched (baq_edges.idaq_table says
which indels a read's table takes)."""
import numpy as np
import pytest

import baq_edges as be

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TABLE = be.boundary_table()
PAD = be.pad_reads()
_ORACLE = {}


def _expected(oracle, r, extended):
    """(lb, ai or None, ad or None) the device must give for read r: the oracle's, with '~' at the indels r's table drops"""
    key = (r["pos0"], tuple(r["cigar"]), r["seq"].tobytes(), r["qual"].tobytes(), extended)
    if key not in _ORACLE:
        lb, ai, ad = oracle.baq_idaq_read(r["pos0"], r["cigar"], r["seq"], r["qual"], be.CONTIG, extended)
        for kind, qpos, _, tracked in be.idaq_table(r, be.CONTIG, be.REF_LEN):
            if not tracked:
                (ai if kind == "I" else ad)[qpos - 1] = ord("~")
        _ORACLE[key] = (lb, ai, ad)
    return _ORACLE[key]


def _check(oracle, caller, reads, extended, what):
    """both batch entry points on `reads` against the oracle -> {read name: (lb, ai, ad) bytes}"""
    import lofreq_amd as la
    plain = la.baq_batch(caller, reads, be.CONTIG, extended=extended)
    both = la.baq_batch(caller, reads, be.CONTIG, extended=extended, idaq=True)
    assert len(plain) == len(both) == len(reads)
    for r, lb0, (lb, ai, ad) in zip(reads, plain, both):
        elb, eai, ead = _expected(oracle, r, extended)
        at = (what, extended, r["name"])
        assert lb0.tobytes() == elb.tobytes(), at
        assert lb.tobytes() == elb.tobytes(), at
        assert (ai is None) == (eai is None) and (ad is None) == (ead is None), at
        assert ai is None or ai.tobytes() == eai.tobytes(), at
        assert ad is None or ad.tobytes() == ead.tobytes(), at
    return both


def _arrays(reads):
    n = len(reads)
    cig = [(l << 4) | be.OPS.index(op) for r in reads for op, l in r["cigar"]]
    return {"n": n, "ref": be.CONTIG, "pos": np.array([r["pos0"] for r in reads], np.int32),
            "cig_off": np.cumsum([0] + [len(r["cigar"]) for r in reads]).astype(np.int64), "cig": np.array(cig or [0], np.uint32),
            "seq_off": np.cumsum([0] + [len(r["seq"]) for r in reads]).astype(np.int64),
            "seq": np.concatenate([r["seq"] for r in reads] + [np.zeros(1, np.uint8)]),
            "qual": np.concatenate([r["qual"] for r in reads] + [np.zeros(1, np.uint8)]),
            "mapq": np.full(n, 60, np.uint8), "rev": np.zeros(n, np.uint8)}


@pytest.mark.parametrize("row", TABLE, ids=be.row_id)
def test_row(caller, oracle, row):
    from lofreq_amd.pileup import ReadSet
    reads = row.reads
    n_bases = sum(len(r["seq"]) for r in reads)
    if row.overflow:
        assert any(not x[3] for r in reads for x in be.idaq_table(r, be.CONTIG, be.REF_LEN))
    for extended in (True, False):
        alone = _check(oracle, caller, reads, extended, "alone")
        _check(oracle, caller, PAD + reads, extended, "behind a wavefront of plain reads")
        _check(oracle, caller, reads[::-1], extended, "reversed")
        # the resident read set: the same routing, another upload path
        for idaq in (False, True):
            rs = ReadSet.from_arrays(caller, _arrays(reads))
            rs.baq(extended=extended, idaq=idaq)
            lb, ai, ad, fl = rs.fetch_tags(idaq=idaq)
            rs.close()
            assert lb[:n_bases].tobytes() == b"".join(x[0].tobytes() for x in alone), (extended, idaq)
            if idaq:
                off = 0
                for r, (_, eai, ead), f in zip(reads, alone, fl):
                    n = len(r["seq"])
                    assert int(f) == (eai is not None) + 2 * (ead is not None), (extended, r["name"])
                    assert ai[off:off + n].tobytes() == (eai.tobytes() if eai is not None else b"~" * n), (extended, r["name"])
                    assert ad[off:off + n].tobytes() == (ead.tobytes() if ead is not None else b"~" * n), (extended, r["name"])
                    off += n
