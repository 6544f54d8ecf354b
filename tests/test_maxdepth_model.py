"""CPU: the -d / --max-depth rule restated in Python (tests/maxdepth_model.py) against the reference's 2.1.4 binary
(tests/golden/maxdepth_*.json): the kept reads give every plpsummary column dump, and the oracle chain on the kept reads
gives every VCF line and test count of `lofreq call -d`."""
import os
import subprocess
import sys

import numpy as np
import pytest

import maxdepth_model as mm
import oracle_chain as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rule_on_the_worked_example():
    """100 x 10, 101 x 4, 150 x 6 (1-based), all 60M: kept per run at -d 3 / 5 / 100"""
    pos = [99] * 10 + [100] * 4 + [149] * 6
    ends = [p + 60 for p in pos]
    assert list(np.add.reduceat(mm.kept(pos, ends, 3), [0, 10, 14])) == [3, 1, 1]
    assert list(np.add.reduceat(mm.kept(pos, ends, 5), [0, 10, 14])) == [5, 1, 1]
    assert list(np.add.reduceat(mm.kept(pos, ends, 100), [0, 10, 14])) == [10, 4, 6]
    # the end boundary: reads of [99, 159) still count at 159, not at 160
    assert list(mm.kept([99] * 3 + [159] * 3, [159] * 3 + [189] * 3, 3)) == [1, 1, 1, 1, 0, 0]
    assert list(mm.kept([99] * 3 + [160] * 3, [159] * 3 + [190] * 3, 3)) == [1, 1, 1, 1, 1, 1]
    # max_depth 0: the first read of every start position only
    assert list(mm.kept([5, 5, 6, 6], [10, 10, 11, 11], 0)) == [1, 0, 1, 0]


def test_stacks_columns_match_plpsummary():
    fx, reads = mm.load("maxdepth_stacks")
    for run in fx["runs"]:
        keep = mm.kept_reads(reads, run["max_depth"])
        kr = [r for r, k in zip(reads, keep) if k]
        assert mm.fwrv_columns(kr) == mm.plpsummary_columns(run), run["max_depth"]
        assert {c["pos0"] for c in run["columns"]} == mm.covered(kr), run["max_depth"]
    # the fixture covers what it claims: a cap that drops reads, positions that only dropped reads cover
    small = fx["runs"][0]
    assert small["max_depth"] == 1 and len(mm.covered(reads) - {c["pos0"] for c in small["columns"]}) > 0


@pytest.mark.parametrize("name", ["maxdepth_stacks", "maxdepth_chain"])
def test_oracle_chain_on_kept_reads_matches_the_binary_vcf(oracle, name):
    fx, reads = mm.load(name)
    ref = fx["genome"].encode()
    oc.add_alnqual_tags(oracle, reads, ref, extended=True, idaq=False)      # per read, before the cap (mplp_func)
    for run in fx["runs"]:
        keep = mm.kept_reads(reads, run["max_depth"])
        kr = [r for r, k in zip(reads, keep) if k]
        kw, ndf = __import__("golden_util").conf_kwargs(run["call_args"])
        out = oc.call_region(oracle, kr, ref, 0, len(ref), kw, call_indels=False, raw_counts_after_minbq=1,
                             no_default_filter=ndf)
        assert out["n_snv_tests"] == run["num_snv_tests"], (run["max_depth"], run["call_args"])
        assert out["lines"] == run["vcf"], (run["max_depth"], run["call_args"])


def test_oracle_chain_with_indels_on_kept_reads_matches_the_binary_vcf(oracle):
    """maxdepth_indel: BI / BD tags, `--call-indels -d 60`: BAQ / IDAQ on every read, the pileups and calls on the kept ones"""
    import golden_util as gu
    fx, R = mm.load_generated("maxdepth_indel")
    P = dict(R)
    oracle.baq_idaq_reads(P, extended=True, idaq=True, procs=1)
    keep = mm.kept_flat(R, fx["max_depth"])
    assert 0 < keep.sum() < R["n"]
    kw, ndf = gu.conf_kwargs(fx["call_args"])
    out = oc.call_region(oracle, mm.subset_flat(P, keep), R["ref"], 0, R["glen"], kw, call_indels=True,
                         no_default_filter=ndf, raw_counts_after_minbq=1)
    assert out["n_snv_tests"] == fx["num_tests"]["snv"] and out["n_indel_tests"] == fx["num_tests"]["indel"]
    assert [gu.strip_hqa(l) for l in out["lines"]] == fx["vcf"]
    assert any("INDEL" in l for l in fx["vcf"])


@pytest.mark.skipif(not os.path.isfile("/root/reference/dist/lofreq_star-2.1.4_linux-x86-64.tgz"),
                    reason="reference dist not mounted")
def test_regenerated_maxdepth_fixtures_are_byte_identical(tmp_path):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    env = dict(os.environ)
    env["LFQ_GOLDEN_OUT"] = str(tmp_path)
    env["PATH"] = "/usr/bin:/bin"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "make_maxdepth_golden.py")], env=env,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    made = sorted(os.listdir(tmp_path))
    assert made == ["maxdepth_c4.json", "maxdepth_chain.json", "maxdepth_indel.json", "maxdepth_stacks.json"]
    for f in made:
        assert open(tmp_path / f, "rb").read() == open(os.path.join(ROOT, "tests", "golden", f), "rb").read(), f
