"""CPU tests of the BAQ oracle: the restated profile HMM against the reference's own
kprobaln_ext.c object (compiled unmodified, oracle/_ref), bit for bit: against its outputs stored in
tests/golden/ref_parts.npz."""
import numpy as np
import pytest

import ref_vectors as rv


@pytest.mark.parametrize("seed", range(6))
def test_hmm_restatement_equals_reference_object(oracle, seed):
    """the restatement on the seeded reads of oracle/ref_vectors.py against what the reference's kpa_ext_glocal returned for
    them (tests/golden/ref_parts.npz; tests/test_ref_parts.py checks the file against the live object where it is built)"""
    n = 0
    for ref, query, qual, bw, runs in rv.kpa_by_seed(rv.load(), seed):
        for d, e, pr, state, q in runs:
            b = oracle.kpa_glocal(ref, query, qual, d, e, bw, use_reference=False)
            assert pr == b[0]
            assert (state == b[1]).all() and (q == b[2]).all()
            n += len(query)
    assert n > 5000


def test_baq_read_perfect_match_and_mismatch(oracle):
    """a perfectly matching read far from the ends keeps high BAQ; extended BAQ is the min of the running
    maxima from both ends of each match block (bam_md_ext.c:431-451)"""
    rng = np.random.default_rng(1)
    genome = "".join(rng.choice(list("ACGT"), 400))
    pos, l = 100, 80
    seq = np.array(["ACGT".index(c) for c in genome[pos:pos + l]], np.uint8)
    qual = np.full(l, 35, np.uint8)
    out = oracle.baq_read(pos, [("M", l)], seq, qual, genome.encode())
    assert out is not None and len(out) == l
    assert out.max() <= 93 + 33 and out.min() >= 33
    plain = oracle.baq_read(pos, [("M", l)], seq, qual, genome.encode(), extended=False)
    assert (out >= plain).all()           # the extension can only raise a base's BAQ
    # soft-clipped and inserted bases are not aligned by the HMM: their BAQ is their base quality (:391-392)
    seq2 = np.concatenate([np.array([0, 0, 0], np.uint8), seq])
    out2 = oracle.baq_read(pos, [("S", 3), ("M", l)], seq2, np.full(l + 3, 35, np.uint8), genome.encode())
    assert (out2[:3] == 35 + 33).all()


@pytest.mark.parametrize("path", __import__("golden_util").baq_fixtures(), ids=lambda p: p.split("/")[-1])
def test_oracle_reproduces_alnqual_lb_tags(oracle, path):
    """orc_baq_read vs the `lb` tags the reference's 2.1.4 binary (`lofreq alnqual`) wrote, byte for byte"""
    import golden_util as gu
    fx, reads = gu.load_baq(path)
    extended = "-e" not in fx["alnqual_args"]
    genome = fx["genome"].encode()
    nbytes = 0
    for r in reads:
        out = oracle.baq_read(r["pos0"], r["cigar"], r["seq"], r["qual"], genome, extended=extended)
        assert r["lb"] is not None and out is not None
        assert out.tobytes() == r["lb"].tobytes(), (r["pos0"], r["cigar"])
        nbytes += len(out)
    assert nbytes > 10000


@pytest.mark.parametrize("path", __import__("golden_util").baq_fixtures(), ids=lambda p: p.split("/")[-1])
def test_oracle_reproduces_alnqual_ai_ad_tags(oracle, path):
    """the indel alignment qualities (idaq, bam_md_ext.c:73-248) vs the ai / ad tags of the 2.1.4 binary"""
    import json
    import golden_util as gu
    fx, reads = gu.load_baq(path)
    raw = json.load(open(path))["reads"]
    extended = "-e" not in fx["alnqual_args"]
    genome = fx["genome"].encode()
    n_tags = 0
    for r, rr in zip(reads, raw):
        lb, ai, ad = oracle.baq_idaq_read(r["pos0"], r["cigar"], r["seq"], r["qual"], genome, extended=extended)
        assert lb.tobytes() == r["lb"].tobytes()
        assert (ai is None) == (rr["ai"] is None) and (ad is None) == (rr["ad"] is None), (r["pos0"], r["cigar"])
        if ai is not None:
            assert ai.tobytes() == rr["ai"].encode(), (r["pos0"], r["cigar"])
            n_tags += 1
        if ad is not None:
            assert ad.tobytes() == rr["ad"].encode(), (r["pos0"], r["cigar"])
            n_tags += 1
    assert n_tags >= 80
