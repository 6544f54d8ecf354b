"""GPU tests: `lofreq faidx` and the whole-contig fetch on the device (lfq_fasta_open, lfq_fasta_index_build, lfq_fasta_fetch) against
tests/fasta_model.py on every row of tests/fasta_edges.py and every text of tests/golden/fasta_binary.json; a parsed foreign index;
the chain lfq_bgzf_inflate -> Fasta.open on the resident bytes with the binary's .fai and .gzi; the hand-over of a fetched contig to a
read set, device to device; `checkref` on the binary's outcomes."""
import numpy as np
import pytest

import fasta_edges as fe
import fasta_model as fm
from test_bed_model import FX, READS
from test_fasta_model import GOLD

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROWS = [{"name": r["name"], "data": r["data"], "fai": r["fai"], "where": r["where"]} for r in fe.ROWS]
ROWS += [{"name": "golden_" + c["name"], "data": c["text"].encode("latin-1"), "fai": None, "where": {}} for c in GOLD["cases"]]
ROWS += [{"name": "stale_" + c["name"], "data": c["new"].encode("latin-1"), "fai": c["fai"].encode("latin-1"), "where": {}}
         for c in GOLD["stale"]]


def _check_row(la, caller, r):
    from lofreq_amd import fasta as lf
    m, fetched = fe.expected(r)
    fa = la.Fasta.open(caller, r["data"])
    try:
        t = la.last_fasta_times(caller)
        assert t["n_from_device"] == 0 and t["n_bytes"] == len(r["data"])
        n_lines = r["data"].count(b"\n") + (1 if r["data"] and not r["data"].endswith(b"\n") else 0)
        assert t["n_lines"] == n_lines
        assert t["n_headers"] == sum(1 for ln in r["data"].split(b"\n") if ln.startswith(b">"))
        if m["status"] != 0:
            with pytest.raises(la.FastaError) as e:
                la.FastaIndex.build(fa)
            assert (e.value.why, e.value.line, e.value.byte) == (m["why"], m["line"], m["byte"])
        else:
            built = la.FastaIndex.build(fa)
            assert built.to_text() == m["fai"]
            assert built.n_duplicates == m["n_dup"]
            assert built.entries == [tuple(e) for e in m["entries"]]
        if r["fai"] is not None:
            idx = la.FastaIndex.from_text(r["fai"])
        elif m["status"] == 0:
            idx = built
        else:
            return
        for e, want, regular in fetched:
            if want is None:
                with pytest.raises(RuntimeError):
                    fa.fetch(idx, e[0])
                continue
            got = fa.fetch(idx, e[0])
            assert bytes(got) == want, (r["name"], e[0])        # case kept
            path = la.last_fasta_times(caller)["fetch_path"]
            assert path == (lf.PATH_NONE if not want else lf.PATH_REGULAR if regular else lf.PATH_GENERAL), (r["name"], e[0])
            if want:                            # the resident copy holds the same bytes
                from test_gpu_maxdepth import _fetch
                assert _fetch(got.d_seq_ptr, got.len).tobytes() == want
    finally:
        fa.close()


@pytest.mark.parametrize("r", ROWS, ids=lambda r: r["name"])
def test_index_and_every_contig_equal_the_model(caller, r):
    import lofreq_amd as la
    _check_row(la, caller, r)


def test_irregular_row_takes_the_general_path_and_its_twin_the_regular(caller):
    import lofreq_amd as la
    from lofreq_amd import fasta as lf
    by = {r["name"]: r for r in fe.ROWS}
    out = {}
    for name in ("irregular_blanks", "regular_twin"):
        fa = la.Fasta.open(caller, by[name]["data"])
        idx = la.FastaIndex.build(fa)
        out[name] = (bytes(fa.fetch(idx, "c1")), la.last_fasta_times(caller)["fetch_path"])
        fa.close()
    assert out["irregular_blanks"][1] == lf.PATH_GENERAL and out["regular_twin"][1] == lf.PATH_REGULAR
    assert out["irregular_blanks"][0] == out["regular_twin"][0] == by["regular_twin"]["where"]["letters"]


def test_the_first_offending_line_is_reported_on_every_run(caller):
    import lofreq_amd as la
    by = {r["name"]: r for r in fe.ROWS}
    for name in ("two_offences", "two_offences_other_order"):
        m = fm.build(by[name]["data"])
        for _ in range(3):
            fa = la.Fasta.open(caller, by[name]["data"])
            with pytest.raises(la.FastaError) as e:
                la.FastaIndex.build(fa)
            fa.close()
            assert (e.value.why, e.value.line, e.value.byte) == (m["why"], m["line"], m["byte"])


@pytest.mark.parametrize("case", GOLD["bgzf"], ids=lambda c: c["name"])
def test_inflate_chain_stays_on_the_device(caller, case):
    import lofreq_amd as la
    view = la.bgzf_inflate_view(caller, bytes.fromhex(case["comp_hex"]))
    assert view.data.tobytes() == case["text"].encode("latin-1")
    fa = la.Fasta.open(caller, view.data)
    assert la.last_fasta_times(caller)["n_from_device"] == 1
    idx = la.FastaIndex.build(fa)
    assert idx.to_text().decode("latin-1") == case["fai"]
    assert la.bgzf_gzi(view).hex() == case["gzi_hex"]
    data = case["text"].encode("latin-1")
    for e in fm.build(data)["entries"]:
        assert bytes(fa.fetch(idx, e[0])) == fm.fetch(data, e)
    fa.close()
    fa = la.Fasta.open(caller, view.data.copy())        # the same bytes elsewhere: across the link
    assert la.last_fasta_times(caller)["n_from_device"] == 0
    fa.close()


def _flat(reads, ref):
    cig, cig_off, seq, qual, seq_off = [], [0], [], [], [0]
    for r in reads:
        cig += [(l << 4) | "MIDNSHP=X".index(o) for o, l in r["cigar"]]
        cig_off.append(len(cig))
        seq.append(np.asarray(r["seq"], np.uint8))
        qual.append(np.asarray(r["qual"], np.uint8))
        seq_off.append(seq_off[-1] + len(seq[-1]))
    return {"n": len(reads), "pos": [r["pos0"] for r in reads], "cig_off": cig_off, "cig": cig, "seq_off": seq_off,
            "seq": np.concatenate(seq), "qual": np.concatenate(qual), "mapq": [r["mapq"] for r in reads],
            "rev": [1 if r["reverse"] else 0 for r in reads], "ref": ref}


def _summary_and_lines(la, caller, rs, name, n):
    from test_gpu_configs import _snv_lines
    summary = la.format_plp_summary(name, rs.plp_summary(0, n))
    rs.baq(extended=True, idaq=False)
    dt = rs.pileup_snv(0, n)
    conf = la.VarcallConf()
    recs, _, _ = caller.call_snvs(dt, conf)
    return summary, [l[2] for l in _snv_lines(la, recs, dt.col_pos, conf, chrom=name)], conf.num_snv_tests


def test_fetched_contig_goes_to_the_read_set_on_the_device(caller):
    import lofreq_amd as la
    assert sum(len(v) for v in READS.values()) == 274 and len(FX["contigs"]) == 2
    text = b"".join(b">" + name.encode() + b"\n" + fe.wrap(FX["genome"][name].encode(), 60) for name, _ in FX["contigs"])
    fa = la.Fasta.open(caller, text)
    idx = la.FastaIndex.build(fa)
    n_lines = 0
    for name, n in FX["contigs"]:
        plain = FX["genome"][name].encode()
        ref = fa.fetch(idx, name)
        assert bytes(ref) == plain and len(ref) == n
        before = la.last_fasta_times(caller)["n_handovers"]
        rs = la.ReadSet.from_arrays(caller, _flat(READS[name], ref))
        assert rs.ref_from_device and la.last_fasta_times(caller)["n_handovers"] == before + 1
        got = _summary_and_lines(la, caller, rs, name, n)
        rs.close()
        rs = la.ReadSet.from_arrays(caller, _flat(READS[name], plain))
        assert not rs.ref_from_device and la.last_fasta_times(caller)["n_handovers"] == before + 1
        want = _summary_and_lines(la, caller, rs, name, n)
        rs.close()
        assert got == want
        assert len(want[0]) > 300
        n_lines += len(want[1])
    assert n_lines > 0
    fa.close()
    # a closed file's contig is no longer recognised
    rs = la.ReadSet.from_arrays(caller, _flat(READS["c1"], FX["genome"]["c1"].encode()))
    assert not rs.ref_from_device
    rs.close()


@pytest.mark.parametrize("case", GOLD["checkref"], ids=lambda c: c["name"])
def test_checkref_on_the_binarys_outcomes(caller, case):
    import lofreq_amd as la
    fa = la.Fasta.open(caller, case["text"].encode("latin-1"))
    idx = la.FastaIndex.build(fa)
    bad, why = la.checkref(idx, [s[0] for s in case["sq"]], [s[1] for s in case["sq"]])
    fa.close()
    assert (bad < 0) == (case["status"] == 0)
    assert (bad, why) == fm.checkref(fm.build(case["text"].encode("latin-1"))["entries"], [s[0] for s in case["sq"]], [s[1] for s in case["sq"]])
    if bad >= 0:
        assert case["sq"][bad][0] in case["messages"][-1] and (why == fm.LENGTH) == ("length mismatch" in case["messages"][-1])
