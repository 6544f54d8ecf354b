"""No GPU: the expected values of tests/test_gpu_readset_uniq.py are right before a device is involved.  The oracle road
(tests/uniq_sites_cases.py) against two plain restatements of the pileup on every row of the case table, and against every
value the 2.1.4 binary stored in tests/golden/uniq_reads.json."""
import numpy as np
import pytest

import golden_util as gu
import uniq_sites_cases as uc


@pytest.mark.parametrize("case", uc.cases(), ids=uc.case_ids())
def test_oracle_sites_agree_with_the_plain_restatements(oracle, case):
    reads, ref = case["reads"], case["ref"]
    pos = [v[0] for v in case["variants"]]
    S = uc.oracle_sites(oracle, reads, ref, pos, case["min_plp_bq"])
    plain = gu.py_pileup(reads, case["min_plp_bq"])
    indel = gu.py_indel_pileup(reads, ref)
    for i, p in enumerate(pos):
        col = plain.get(p, {})
        o0, o1 = int(S["col_off"][i]), int(S["col_off"][i + 1])
        assert o1 - o0 == sum(len(x) for x in col.values()) == S["nb"][i], (case["name"], p)
        for code, letter in enumerate("ACGTN"):
            sel = (S["nt"][o0:o1] & 7) == code
            want = col.get(letter, [])
            assert S["bq"][o0:o1][sel].tolist() == [min(int(reads[r]["qual"][q]), 93) for r, q in want], (case["name"], p, letter)
            assert S["mq"][o0:o1][sel].tolist() == [reads[r]["mapq"] for r, _ in want]
            assert (S["nt"][o0:o1][sel] >> 3).tolist() == [int(reads[r]["reverse"]) for r, _ in want]
        c = indel.get(p)
        assert S["cov"][i] == (c["cov"] if c else 0) and S["tails"][i] == (c["tails"] if c else 0), (case["name"], p)
        for s in (0, 1):
            assert S["events"][i][s] == ({k: len(v) for k, v in c["ev"][s].items()} if c else {}), (case["name"], p, s)
        assert S["ref_base"][i] == uc.ref_base_of(ref, p)


def test_case_table_covers_what_it_says(oracle):
    """the rows reach the situations they are there for (window sizes, tails, events, empty columns)"""
    by = {c["name"]: c for c in uc.cases()}
    S = uc.oracle_sites(oracle, by["windows"]["reads"], by["windows"]["ref"], [v[0] for v in by["windows"]["variants"]])
    assert sorted(S["cov"].tolist()) == [0, 0, 1, 63, 64, 65, 128, 129]
    c = by["long_window"]
    S = uc.oracle_sites(oracle, c["reads"], c["ref"], [350, 380])
    assert S["cov"].tolist() == [1, 71]
    assert len(by["wide"]["reads"]) > 65 * 65
    for name, cov in (("all_tails", [6, 0, 0]), ("all_but_one_tails", [7, 1, 1])):
        c = by[name]
        S = uc.oracle_sites(oracle, c["reads"], c["ref"], [v[0] for v in c["variants"]])
        U = uc.oracle_uniq(oracle, S, c["variants"])
        assert U["coverage"].tolist()[:3] == cov and S["nb"][1] > 0
        assert (U["uq"][:3] >= 0).tolist() == [x > 0 for x in cov]
    c = by["del_keys"]
    S = uc.oracle_sites(oracle, c["reads"], c["ref"], [v[0] for v in c["variants"]])
    U = uc.oracle_uniq(oracle, S, c["variants"])
    assert U["alt_count"][:8].tolist() == [3, 0, 1, 0, 2, 1, 1, 0]
    c = by["in_ops"]
    S = uc.oracle_sites(oracle, c["reads"], c["ref"], [v[0] for v in c["variants"]])
    U = uc.oracle_uniq(oracle, S, c["variants"])
    assert U["alt_count"][9:].tolist() == [3, 1, 1, 0, 0, 4, 0, 1, 0]
    c = by["ambiguity"]
    S = uc.oracle_sites(oracle, c["reads"], c["ref"], [v[0] for v in c["variants"]])
    assert uc.oracle_uniq(oracle, S, c["variants"])["alt_count"][:6].tolist() == [2, 1, 1, 1, 0, 0]
    c = by["quals"]
    S = uc.oracle_sites(oracle, c["reads"], c["ref"], [105])
    assert S["cov"][0] == 5 and sorted(S["bq"].tolist()) == [3, 93, 93, 93]


@pytest.mark.parametrize("run", ["default", "detlim", "unifreq"])
def test_oracle_road_equals_the_reference_binary(oracle, run):
    """uniq_reads.json: UQ= (or its absence), the UNIQ flag and PASS / uq_fdr of all three runs of the 2.1.4 binary"""
    fx, ref, reads, var = uc.load_uniq_reads()
    assert len(reads) < len(fx["reads"])                    # uniq's read filter drops some, here
    S = uc.oracle_sites(oracle, reads, ref, [v[0] for v in var])
    U = uc.oracle_uniq(oracle, S, var, af=0.5 if run == "unifreq" else None)
    uq, flags, passed = uc.binary_run(fx, run)
    if run == "detlim":
        assert U["detectable"].astype(bool).tolist() == flags
        assert all(x == -1 for x in uq)
    else:
        assert U["uq"].tolist() == uq
        assert not any(flags)
        assert oracle.uniq_mtc(U["uq"], fx["mtc"], fx["alpha"], 0).tolist() == passed
