"""CPU: the plain-Python model of `lofreq indelqual` (tests/indelqual_model.py) gives the BI and BD strings the reference's 2.1.4
binary wrote for every fixture read in every mode (tests/golden/indelqual_*.json, tests/make_indelqual_golden.py), and the
fixtures are what they claim to be: every letter of the Dindel table, every operation, the contig's end, runs beyond 18, N runs
and lower-case reference all occur; the end-to-end fixture has indel calls, and they depend on the Dindel qualities."""
import json
import os

import pytest

import golden_reads as gr
import golden_util as gu
import indelqual_model as im
import indelqual_reads as ir
import viterbi_reads as vr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILIES = ("indelqual_small", "indelqual_shapes")


def load_family(name):
    """-> (fixture, genome, reads as dicts {name, pos0, cigar [(op, len)], l_qseq})"""
    fx = json.load(open(os.path.join(GOLDEN, name + ".json")))
    if "reads" in fx:
        reads = [{"name": n, "pos0": p, "cigar": gu.parse_cigar(c), "l_qseq": l} for n, p, c, l in fx["reads"]]
        return fx, fx["genome"], reads
    g = fx["generator"]
    assert g["version"] == ir.GENERATOR_VERSION, "fixture written by another version of tests/indelqual_reads.py"
    R = ir.make(**g["params"])
    assert vr.sha256(vr.sam_text(R["genome"], R["reads"])) == fx["sam_sha256"]
    return fx, R["genome"], [{"name": r["name"], "pos0": r["pos0"], "cigar": r["cigar"], "l_qseq": len(r["seq"])} for r in R["reads"]]


def model_tags(genome, reads, mode):
    if mode == "dindel":
        table = im.dindel_table(genome)
        out = [im.dindel_read(table, r["pos0"], r["cigar"]) for r in reads]
        return [(s, s) for s in out]
    return [im.uniform_read(r["l_qseq"], *ir.mode_quals(mode)) for r in reads]


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("mode", ir.MODES)
def test_model_gives_the_binarys_tags(name, mode):
    fx, genome, reads = load_family(name)
    assert len(reads) == fx["n_reads"] and set(fx["results"]) == set(ir.MODES)
    got = model_tags(genome, reads, mode)
    for i, r in enumerate(reads):
        assert got[i] == ir.fixture_tags(fx["results"][mode], i), (name, mode, r["name"])
        assert len(got[i][0]) == len(got[i][1]) == r["l_qseq"]


def test_uniform_clamps():
    """ENCODE_Q (lofreq_indelqual.c:66)"""
    fx = json.load(open(os.path.join(GOLDEN, "indelqual_small.json")))
    assert (fx["results"]["u40"]["bi_byte"], fx["results"]["u40"]["bd_byte"]) == ("I", "I")
    assert (fx["results"]["u40,100"]["bi_byte"], fx["results"]["u40,100"]["bd_byte"]) == ("I", "~")
    assert (fx["results"]["u-5"]["bi_byte"], fx["results"]["u-5"]["bd_byte"]) == ("!", "!")


def test_fixtures_exercise_the_rule():
    letters, ops = set(), set()
    ends_on_last = long_run = n_run = lower = False
    for name in FAMILIES:
        fx, genome, reads = load_family(name)
        res = fx["results"]["dindel"]
        assert res["bd"] is None                                    # BI == BD in every record the binary wrote
        for i, r in enumerate(reads):
            letters |= set(ir.fixture_tags(res, i)[0])
            ops |= {o for o, _ in r["cigar"]}
            end = r["pos0"] + sum(l for o, l in r["cigar"] if o in "M=XD")
            ends_on_last = ends_on_last or end == len(genome)
        counts = im.homopolymer_counts(genome)
        long_run = long_run or max(counts) > 18
        n_run = n_run or any(c >= 2 and genome[p] == "N" for p, c in enumerate(counts))
        lower = lower or any(c.islower() for c in genome)
    assert letters == set(im.DINDELQ) and len(letters) == 15        # the 14 quality letters of the table and '!'
    assert ops == set("MIDSH=X")
    assert ends_on_last and long_run and n_run and lower


def test_end_to_end_fixture():
    fx = json.load(open(os.path.join(GOLDEN, "indelqual_e2e.json")))
    R = gr.make(**fx["generator"]["params"])
    R["bi"] = R["bd"] = None
    assert gr.sam_sha256(R) == fx["sam_sha256"] and R["n"] == fx["n_reads"]
    indel = [l for l in fx["vcf"] if "INDEL" in l.split("\t")[7]]
    assert len(indel) == fx["n_indel_lines"] >= 20
    assert fx["num_tests"]["indel"] >= len(indel) and fx["num_tests"]["snv"] > 0
    # the calls depend on the qualities: the lines differ from what uniform 40 gives for the same reads, at 20 sites or more
    # (47 of the 49 do; the two others have the same QUAL either way)
    assert len(fx["indel_lines_after_uniform_40"]) > 0
    assert indel != fx["indel_lines_after_uniform_40"]
    assert len(set(indel) - set(fx["indel_lines_after_uniform_40"])) >= 20


def test_model_refuses_what_the_reference_dies_on():
    with pytest.raises(ValueError):
        im.dindel_read(im.dindel_table("ACGT" * 20), 3, [("M", 10), ("N", 5), ("M", 10)])
    with pytest.raises(ValueError):
        im.dindel_read(im.dindel_table("ACGT" * 20), 3, [("M", 10), ("P", 1), ("M", 10)])


def test_rle_round_trip():
    for s in ("", "M", "MMMM!L", "99988,,776", "~" * 300, "!MMMLKEC@=<;:988776"):
        assert im.unrle(im.rle(s)) == s
