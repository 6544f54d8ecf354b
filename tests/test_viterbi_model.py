"""CPU: `lofreq viterbi` restated in Python doubles (tests/viterbi_model.py) against the reference's 2.1.4 binary
(tests/golden/viterbi_*.json, written by tests/make_viterbi_golden.py): position and CIGAR of EVERY fixture read, with the
default -q and with -q 20.  Integers and strings, no tolerance."""
import multiprocessing
import os

import viterbi_model as vm
import viterbi_reads as vr

DEF_QUALS = (-1, 20)


def fixture_reads(name):
    fx = vm.load(name)
    if "reads" in fx:
        reads = [{"name": n, "pos0": p, "cigar": vm.parse_cigar(c), "seq": s, "qual": [ord(ch) - 33 for ch in q], "shape": sh}
                 for n, p, c, s, q, sh in fx["reads"]]
        return fx, fx["genome"], reads
    R = vr.make(**fx["generator"]["params"])
    return fx, R["genome"], R["reads"]


def model_results(genome, reads, def_quals=DEF_QUALS):
    """{def_qual: [(pos0, cigar string, status)]}; a read without a base of quality 2 cannot depend on -q (viterbi.c:188-192)
    and is computed once"""
    jobs, slot = [], {}
    for dq in def_quals:
        for i, r in enumerate(reads):
            key = (i, dq if vr.has_q2(r) else None)
            if key not in slot:
                slot[key] = len(jobs)
                jobs.append((vr.lib_read(r), genome, dq))
    n_proc = max(1, min(16, len(os.sched_getaffinity(0))))
    if n_proc > 1 and len(jobs) > 200:
        with multiprocessing.get_context("spawn").Pool(n_proc) as pool:
            done = pool.map(vm.realign_job, jobs, chunksize=16)
    else:
        done = [vm.realign_job(j) for j in jobs]
    out = {}
    for dq in def_quals:
        res = [done[slot[(i, dq if vr.has_q2(r) else None)]] for i, r in enumerate(reads)]
        out[dq] = [(p, vm.cigar_str(c), s) for p, c, s in res]
    return out


def test_int_median_and_left_alignment():
    assert vm.int_median([]) == 0 and vm.int_median([7]) == 7 and vm.int_median([30, 33]) == 31
    assert vm.int_median([40, 2, 11]) == 11 and vm.int_median([1, 2, 3, 4]) == 2
    # the three calls of viterbi_test (viterbi.c:339-341)
    assert vm.left_align_indels(list("CCATATGG"), list("CCAT**GG")) == "MMDDMMMM"
    assert vm.left_align_indels(list("CCAT**GG"), list("CCATATGG")) == "MMIIMMMM"
    assert vm.left_align_indels(list("CCATATGG*CC"), list("CCAT**GGGCC")) == "MMDDMMIMMMM"
    # a shift at index 0 (the reference then looks at index -1)
    assert vm.left_align_indels(list("A*CG"), list("AACG")) == "IMMM"


def test_worked_example_of_viterbi_test():
    """viterbi("CCATATGG", "CCATGG", "??????", ., 20) (viterbi.c:336): the deletion ends up at the left of the repeat"""
    k, aln = vm.viterbi("CCATATGG", "CCATGG", [30] * 6, 20)
    assert (k, aln) == (0, "MMDDMMMM")


def _check(name):
    fx, genome, reads = fixture_reads(name)
    assert len(reads) == fx["n_reads"]
    assert vr.sha256(vr.sam_text(genome, reads)) == fx["sam_sha256"]
    got = model_results(genome, reads)
    for dq in DEF_QUALS:
        want = fx["results"][str(dq)]
        assert len(want) == len(reads)                      # no read is left out
        bad = [(r["name"], dq, g[:2], tuple(w)) for r, g, w in zip(reads, got[dq], want) if list(g[:2]) != w]
        assert not bad, (len(bad), bad[:5])
    return fx, genome, reads, got


def test_small_fixture_every_read_matches_the_binary():
    fx, genome, reads, got = _check("viterbi_small")
    assert fx == vm.load("viterbi_small") and len(reads) >= 300
    # the four kinds of read that are left alone are there, and are left alone
    st = {r["shape"]: set() for r in reads}
    for r, g in zip(reads, got[-1]):
        st[r["shape"]].add(g[2])
    assert st["plain"] == {vm.NO_INDEL} and st["hclip"] == {vm.SKIPPED_OP} and st["nop"] == {vm.SKIPPED_OP}
    assert st["allq2"] == {vm.ALL_Q2}


def test_shapes_fixture_every_read_matches_the_binary():
    fx, genome, reads, got = _check("viterbi_shapes")
    assert len(reads) >= 2000
    # what the fixture claims to cover
    cig = ["".join(o for o, _ in r["cigar"]) for r in reads]
    indel = [r for r in reads if r["shape"] not in ("plain", "hclip", "nop", "allq2")]
    assert any(c.startswith("I") for c in cig) and any(c.endswith("I") for c in cig)
    assert any(c.startswith("S") for c in cig) and any(c.endswith("S") for c in cig)
    assert any("=" in c for c in cig) and any("X" in c for c in cig)
    assert {36, 75, 150, 250} <= {len(r["seq"]) for r in indel} and any(len(r["seq"]) >= 300 for r in indel)
    assert any(l == 30 for r in indel for o, l in r["cigar"] if o == "D")
    assert any(0 in r["qual"] for r in indel) and any(r["qual"].count(2) >= 5 for r in indel)
    assert any("N" in r["seq"] for r in indel) and any(set(r["seq"]) & set("MRSVWYHKDB") for r in indel)
    assert "N" in genome and any(c.islower() for c in genome)
    assert any(r["pos0"] < 10 for r in indel)
    assert any(r["pos0"] + sum(l for o, l in r["cigar"] if o in "MD=X") > len(genome) - 10 for r in indel)
    # -q matters to some read
    assert any(a != b for a, b in zip(fx["results"]["-1"], fx["results"]["20"]))


def test_fixtures_are_not_vacuous():
    """on the binary's recorded output alone: at least 20 % of the reads with an indel come back with another CIGAR, and at
    least 20 reads at another position"""
    for name in ("viterbi_small", "viterbi_shapes"):
        fx, genome, reads = fixture_reads(name)
        for dq in DEF_QUALS:
            want = fx["results"][str(dq)]
            with_indel = [(r, w) for r, w in zip(reads, want) if any(o in "ID" for o, _ in r["cigar"])]
            new_cigar = sum(1 for r, w in with_indel if vm.cigar_str(r["cigar"]) != w[1])
            moved = sum(1 for r, w in zip(reads, want) if r["pos0"] != w[0])
            assert new_cigar * 5 >= len(with_indel) > 0, (name, dq, new_cigar, len(with_indel))
            assert moved >= 20, (name, dq, moved)
            # every read of the "shifted" kind was moved by the binary
            shifted = [(r, w) for r, w in zip(reads, want) if r["shape"] == "shifted"]
            assert shifted and all(r["pos0"] != w[0] for r, w in shifted)
