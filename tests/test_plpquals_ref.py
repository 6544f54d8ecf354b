"""CPU tests: the plain restatement of plp_summary's quality lines (tests/plpquals_ref.py) against the reference's own binary --
the complete text of tests/golden/plpquals_indel.json, plpquals_srcq.json and plpquals_deep.json character for character -- and the
fixtures hold what they are for.  This holds the checker the GPU tests and the edge table use."""
import json

import pytest

import golden_util as gu
import plpquals_ref as Q

GOLDENS = ("plpquals_indel", "plpquals_srcq", "plpquals_deep")


def _lines(text, title, heads=None):
    """[(head, [values])] of the quality lines with this title"""
    out = []
    for line in text.split("\n"):
        f = line.split("\t")
        if line.startswith("  ") and len(f) == 3 and f[1] == title + " =" and (heads is None or heads(f[0].strip())):
            out.append((f[0].strip(), [int(v) for v in f[2].split()]))
    return out


@pytest.mark.parametrize("name", GOLDENS)
def test_the_complete_text_of_the_binary(oracle, name):
    fx, reads, blocks = Q.load_golden(name)
    assert fx["not_comparable"] == [] and fx["reference_binary"].startswith("lofreq 2.1.4")
    genome = fx["genome"]
    flag = Q.flag_of(fx)
    if flag & Q.LFQ_USE_SQ:
        for r, s in zip(reads, Q.source_quals(oracle, reads, genome)):
            r["sq"] = s
    got = Q.text(fx["chrom"], reads, genome, 0, len(genome), flag)
    assert len(got) == len(blocks) >= 20
    for g, w in zip(got, blocks):
        assert g == w
    assert "".join(got) == fx["text"]


def test_the_goldens_hold_what_they_are_for():
    fx = {n: json.load(open(gu.GOLDEN_DIR + "/%s.json" % n)) for n in GOLDENS}
    for f in fx.values():
        assert len(json.dumps(f, separators=(",", ":"))) < 120 * 1024
        assert all(r[8] is not None for r in f["reads"])                    # every read went through alnqual: an lb tag
    nt, ev = (lambda h: h in "ACGTN"), (lambda h: h[0] in "+-" and h[1:] != "0")
    ind = fx["plpquals_indel"]["text"]
    assert any(v != -1 for _, vals in _lines(ind, "AQ") for v in vals)      # an AQ other than -1
    assert _lines(ind, "IQ", ev) and _lines(ind, "IDQ", ev)                 # insertion and deletion events
    assert "\tSQ =" not in "".join(l for l in ind.split("\n") if l[2:3] in "ACGTN" and l.startswith("  "))   # no -s: no SQ line of a nucleotide
    # a "+0" line with values at a column without any event
    blocks = [b for b in ind.split("\n\n") if b]
    quiet = [b for b in blocks if "\tins:0\tdels:0\t" in b.split("\n")[0]]
    assert quiet and all(len(_lines(b, "IDQ", lambda h: h == "+0")[0][1]) > 0 for b in quiet)
    assert all(not _lines(b, "IQ") and not _lines(b, "AQ") for b in quiet)
    mqs = {v for _, vals in _lines(ind, "MQ") for v in vals} | {v for _, vals in _lines(fx["plpquals_deep"]["text"], "MQ") for v in vals}
    assert {0, 255} <= mqs
    sq = fx["plpquals_srcq"]["text"]
    assert fx["plpquals_srcq"]["args"] == ["-s"]
    assert any(49314 in vals for _, vals in _lines(sq, "SQ", nt)) and any(49314 in vals for _, vals in _lines(sq, "SQ", ev))
    assert any(0 in vals for _, vals in _lines(sq, "SQ"))
    deep = fx["plpquals_deep"]
    assert len(deep["reads"]) >= 130 and all(len(r[4]) <= 12 for r in deep["reads"]) and len(deep["genome"]) <= 24
    best = 0
    for b in [b for b in deep["text"].split("\n\n") if b]:
        groups = [len(vals) for _, vals in _lines(b, "BQ", nt)]
        if sum(groups) >= 129:
            best = max(best, max(groups))
    assert best > 64                                                        # a column >= 129 deep with a group of more than 64


def test_grouping_tracks_is_grouping_reads():
    """the two statements of the restatement agree: group_tracks on tracks made from the reads' columns gives the nucleotide lines"""
    import numpy as np
    fx, reads, blocks = Q.load_golden("plpquals_deep")
    genome = fx["genome"]
    cols = Q.columns(reads, genome, 0, len(genome))
    # tracks in pileup order, as gu.py_pileup files them ... rebuilt here from the walk itself
    flat = {p: [] for p in cols}
    import plpsummary_ref as ref
    cur = [ref.Cursor(r) for r in reads]
    for p in sorted(cols):
        for r, c in zip(reads, cur):
            if r["pos0"] > p or c.end <= p:
                continue
            is_del, qpos, _, _, _ = c.entry(p)
            if not is_del and r["qual"][qpos] >= 3:
                flat[p].append((min(int(r["seq"][qpos]), 4) | (8 if r["reverse"] else 0), int(r["qual"][qpos]),
                                int(r["lb"][qpos]) - 33, r["mapq"]))
    ps = sorted(cols)
    off = np.zeros(len(ps) + 1, np.uint64)
    off[1:] = np.cumsum([len(flat[p]) for p in ps])
    tr = [np.array([o[k] for p in ps for o in flat[p]], np.uint8) for k in range(4)]
    g = Q.group_tracks(tr[0], tr[1], tr[2], tr[3], None, off, 0, len(ps))
    for i, p in enumerate(ps):
        assert Q.format_grouped(*g, i, Q.LFQ_USE_BAQ) == Q.format_nt(cols[p]["nt"])
