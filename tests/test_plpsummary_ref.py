"""CPU tests: the plain restatement of plp_summary's header line (tests/plpsummary_ref.py) against the reference's own binary --
every header line of tests/golden/plpsummary_snv.json and plpsummary_indel.json byte for byte, and the cons / fwrv / num_tails /
hrun / num_ins / num_dels values the older fixtures of the same binary already carry.  This holds the checker the GPU tests use."""
import json

import pytest

import golden_util as gu
import plpsummary_ref as ref

GOLDENS = ("plpsummary_snv", "plpsummary_indel")


@pytest.mark.parametrize("name", GOLDENS)
def test_every_header_line_of_the_binary(name):
    fx, reads = ref.load_golden(name)
    assert fx["not_comparable"] == []
    genome = fx["genome"]
    got = ref.lines(fx["chrom"], reads, genome, 0, len(genome))
    assert len(got) == len(fx["lines"]) > 300
    for g, w in zip(got, fx["lines"]):
        assert g == w
    assert got == fx["lines"]


def test_the_goldens_hold_what_they_are_for():
    snv = json.load(open(gu.GOLDEN_DIR + "/plpsummary_snv.json"))
    f = [l.rstrip("\n").split("\t") for l in snv["lines"]]
    assert sum(1 for x in f if x[8] != "N:0/0") >= 20                      # N bases
    assert sum(1 for x in f if x[2] != x[3]) >= 2                          # planted variants that are the consensus
    depth = [sum(int(v) for t in x[4:9] for v in t.split(":")[1].split("/")) for x in f]
    assert max(depth) > 64                                                 # more than one 64-read round of the kernel
    ind = json.load(open(gu.GOLDEN_DIR + "/plpsummary_indel.json"))
    cons = [l.split("\t")[3] for l in ind["lines"]]
    assert any(c[0] == "+" for c in cons) and any(c[0] == "-" for c in cons)
    assert any(int(l.split("\t")[11].split(":")[1]) > 0 and l.split("\t")[3][0] not in "+-" for l in ind["lines"])
    for fx in (snv, ind):
        assert len(json.dumps(fx, separators=(",", ":"))) < 120 * 1024


@pytest.mark.parametrize("path", gu.plpindel_fixtures(), ids=lambda p: p.split("/")[-1])
def test_cons_tails_hrun_of_the_plpindel_fixtures(path):
    fx, reads = gu.load_plpindel(path)
    genome = fx["genome"]
    cols = {c["pos0"]: c for c in ref.summarize(reads, genome, 0, len(genome))}
    assert fx["columns"]
    for w in fx["columns"]:
        c = cols[w["pos0"]]
        assert c["cons"] == w["cons"], w["pos0"]
        assert (c["ref"], c["tails"], c["hrun"], c["ins"], c["dels"], c["coverage"]) == \
            (w["ref"], w["num_tails"], w["hrun"], w["num_ins"], w["num_dels"], w["coverage_plp"]), w["pos0"]


@pytest.mark.parametrize("path", gu.pileup_fixtures(), ids=lambda p: p.split("/")[-1])
def test_fwrv_of_the_pileup_fixtures(path):
    fx = json.load(open(path))
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    import numpy as np
    reads = [{"pos0": r[0], "cigar": gu.parse_cigar(r[3]), "seq": np.array([code.get(c, 4) for c in r[4]], np.uint8),
              "qual": np.array([ord(c) - 33 for c in r[5]], np.uint8), "mapq": r[2], "reverse": bool(r[1] & 16)}
             for r in fx["reads"]]
    genome = fx["genome"]
    cols = ref.summarize(reads, genome, 0, len(genome))
    assert [c["pos0"] for c in cols] == [w["pos0"] for w in fx["columns"]]
    for c, w in zip(cols, fx["columns"]):
        assert c["ref"] == w["ref"]
        for i, nt in enumerate(ref.NT4):
            assert [c["fw"][i], c["rv"][i]] == w["fwrv"][nt], (w["pos0"], nt)
