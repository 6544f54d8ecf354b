"""GPU tests: VCF text parsed on the device (lfq_vcf_open and what reads the parsed file) and `lofreq vcfset` (lfq_vcfset) against
tests/vcf_model.py on every row of tests/vcf_edges.py: the record table, header, filter_vars (af bit-equal), uniq_variants; keep, counts
and text of every vcfset row; every refusal twice; the -S mask with and without a BED, accumulated, and through
lfq_readset_source_qual; the device-to-device road behind lfq_bgzf_inflate; the chain from lfq_format_vcf's records; what is launched."""
import struct

import numpy as np
import pytest

import bai_model as bm
import vcf_edges as ve
import vcf_model as vm

from test_vcf_model import GOLD, same

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
BINARY = {s["name"]: s for s in GOLD["sets"]}


def _open_expect(la, caller, r):
    try:
        return vm.parse(r["data"], r["mode"]), None
    except vm.Refused as e:
        return None, e


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _check_table(la, v, p):
    assert v.n_records == len(p.recs) and v.n_lines_behind == p.behind
    assert v.header() == (p.header, p.hdr_line >= 0)
    t = v.records()
    want = vm.table(p)
    assert t["line"].tolist() == [w[0] for w in want]
    assert t["pos"].tolist() == [w[1] for w in want]
    assert t["qual"].tolist() == [w[2] for w in want]
    assert (t["flags"] & 31).tolist() == [w[3] for w in want]
    assert t["n_fields"].tolist() == [w[4] for w in want]
    assert t["field_off"].tolist() == [w[5] for w in want]
    assert t["run_id"].tolist() == [r.run for r in p.recs]
    assert [(n, int(b)) for n, b in zip(t["run_name"], t["run_begin"])] == p.runs and int(t["run_begin"][-1]) == len(p.recs)
    if len(p.lines):
        assert t["line_start"][:-1].tolist() == [s for s, _ in p.lines]


@pytest.mark.parametrize("r", [r for r in ve.OPEN if "refused" not in r["where"]], ids=lambda r: r["name"])
def test_table_header_filter_vars_and_uniq_variants_equal_the_model(caller, r):
    import lofreq_amd as la
    p = vm.parse(r["data"], r["mode"])
    v = la.Vcf.open(caller, r["data"], tabix=r["mode"] == vm.TABIX)
    try:
        t = la.last_vcf_times(caller)
        assert t["n_from_device"] == 0 and t["n_bytes"] == len(r["data"]) and t["n_lines"] == len(p.lines)
        _check_table(la, v, p)
        got = v.filter_vars()
        want = vm.filter_vars(p)
        assert [tuple(int(x) for x in (g["is_indel"], g["qual"], g["dp"], g["sb"], g["alt_fw"], g["alt_rv"])) for g in got] == [w[:6] for w in want]
        assert [_bits(float(g["af"])) for g in got] == [_bits(w[6]) for w in want]
        for chrom in sorted({x.chrom for x in p.recs})[:3]:
            for only_unfiltered, uni in ((True, 0.5), (False, 0.5), (True, 0.0)):
                try:
                    w = vm.uniq_variants(p, chrom, only_unfiltered, uni)
                except vm.Refused as e:
                    with pytest.raises(la.VcfError) as ge:
                        v.uniq_variants(chrom, only_unfiltered, uni)
                    assert ge.value.line == e.line
                    continue
                g = v.uniq_variants(chrom, only_unfiltered, uni)
                assert (g["line"].tolist(), g["pos"].tolist(), g["ref"], g["alt"], g["indel_key"].tolist()) == (
                    [x[0] for x in w], [x[1] for x in w], [x[2] for x in w], [x[3] for x in w], [x[4] for x in w])
                assert [_bits(float(a)) for a in g["af"]] == [_bits(x[5]) for x in w]
    finally:
        v.close()


@pytest.mark.parametrize("r", ve.SETS, ids=lambda r: r["name"])
def test_vcfset_keep_counts_and_text_equal_the_model(caller, r):
    import lofreq_amd as la
    want = ve.expected_set(r)
    c = r["conf"]
    opened = []
    try:
        for _ in range(2 if "why" in want else 1):      # a refusal: the same answer on two consecutive runs
            for v in opened:
                v.close()
            opened = [la.Vcf.open(caller, r["one"])]
            two = None
            if r["two"] is not None:
                two = la.Vcf.open(caller, r["two"], tabix=True, file=1)
                opened.append(two)
            more = [la.Vcf.open(caller, m) for m in r["more"]]
            opened += more
            kw = dict(op=c["op"], only_passed=c["only_passed"], only_pos=c["only_pos"], only_snvs=c["only_snvs"], only_indels=c["only_indels"],
                      count_only=c["count_only"], add_info=c["add"] or None)
            if "why" in want:
                with pytest.raises(la.VcfError) as e:
                    la.vcfset(opened[0], two, more, **kw)
                assert (e.value.why, e.value.file, e.value.line) == (want["why"], want["file"] + (1 if want["file"] else 0), want["line"])
                continue
            got = la.vcfset(opened[0], two, more, **kw)
            assert [got["n_vars1"], got["n_ignored"], got["n_out"]] == want["counts"]
            assert got["keep"].tolist() == want["keep"]
            assert got["text"] == bytes.fromhex(want["text"])
            gold = BINARY.get(r["name"])                # the 2.1.4 binary's own output, where the fixture has the row
            if gold is not None:
                assert gold["status"] == 0 and same(gold["out"], b"%d\n" % got["n_out"] if c["count_only"] else got["text"])
            t = la.last_vcf_times(caller)
            if c["count_only"]:
                assert got["text"] == b"" and t["n_set_launches"] == sum(1 for v in [opened[0]] + (more if c["op"] == vm.CONCAT else []) if v.n_records)
    finally:
        for v in opened:
            v.close()


@pytest.mark.parametrize("r", [r for r in ve.OPEN if "refused" in r["where"]], ids=lambda r: r["name"])
def test_every_refusal_twice(caller, r):
    import lofreq_amd as la
    _, want = _open_expect(la, caller, r)
    for _ in range(2):
        with pytest.raises(la.VcfError) as e:
            la.Vcf.open(caller, r["data"], tabix=r["mode"] == vm.TABIX)
        assert (e.value.why, e.value.line) == (want.why, want.line)


def test_ign_mask_equals_the_model_and_feeds_source_qual(caller):
    import lofreq_amd as la
    from test_bed_model import FX, READS
    from test_gpu_fasta import _flat
    for r in ve.MASKS:
        v = la.Vcf.open(caller, r["data"])
        bed = None
        if r["bed"] is not None:
            bed = la.Bed.parse(b"".join(b"%s\t%d\t%d\n" % (r["chrom"], b, e) for b, e in r["bed"]) or b"other\t1\t2\n")
        got = v.ign_mask(r["chrom"], r["ref_len"], bed)
        assert np.flatnonzero(got).tolist() == vm.ign_mask(vm.parse(r["data"]), r["chrom"], r["ref_len"], r["bed"]), r["name"]
        again = v.ign_mask(r["chrom"], r["ref_len"], None, mask=got)        # accumulates: ORs into the caller's array
        assert np.flatnonzero(again).tolist() == vm.ign_mask(vm.parse(r["data"]), r["chrom"], r["ref_len"], None)
        v.close()
    # two -S files on a real contig, then the read set's source quality with the library's mask and with the model's
    name, n = FX["contigs"][0]
    ref = FX["genome"][name].encode()
    files = [ve.HEAD + b"".join(ve.rec(name.encode(), p) for p in range(3, n + 3, 7)), ve.HEAD + ve.rec(name.encode(), 1) + ve.rec(name.encode(), n)]
    mask, want = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for d in files:
        v = la.Vcf.open(caller, d)
        v.ign_mask(name, n, None, mask=mask)
        v.close()
        want[vm.ign_mask(vm.parse(d), name.encode(), n)] = 1
    assert np.array_equal(mask, want) and mask[0] == 1 and mask[n - 1] == 1 and 2 < int(mask.sum()) < n
    rs = la.ReadSet.from_arrays(caller, _flat(READS[name], ref))
    a, b = rs.source_qual(ign=mask).copy(), rs.source_qual(ign=want).copy()
    rs.close()
    assert np.array_equal(a, b)


def test_inflated_vcf_stays_on_the_device(caller):
    import lofreq_amd as la
    by = {r["name"]: r for r in ve.OPEN}
    data = by["mixed_rules"]["data"]
    comp = bm.bgzf_file(data, [100, 101, 700])
    view = la.bgzf_inflate_view(caller, comp)
    assert view.data.tobytes() == data
    v = la.Vcf.open(caller, view.data)
    assert la.last_vcf_times(caller)["n_from_device"] > 0
    _check_table(la, v, vm.parse(data))
    v.close()
    v = la.Vcf.open(caller, view.data.copy())           # the same bytes elsewhere: across the link
    assert la.last_vcf_times(caller)["n_from_device"] == 0
    v.close()


def test_chain_from_called_records_to_filter_and_uniq(caller):
    import ctypes as C
    import lofreq_amd as la
    from lofreq_amd import _lib
    from test_bed_model import FX, READS
    from test_gpu_fasta import _flat
    name, n = FX["contigs"][0]
    ref = FX["genome"][name].encode()
    rs = la.ReadSet.from_arrays(caller, _flat(READS[name], ref))
    rs.baq(extended=True, idaq=False)
    dt = rs.pileup_snv(0, n)
    conf = la.VarcallConf()
    recs, _, _ = caller.call_snvs(dt, conf)
    assert len(recs) > 0
    pos0 = np.asarray([int(dt.col_pos[int(r["col"])]) for r in recs], np.int64)
    text = la.write_vcf_header().encode() + la.format_vcf(recs, name, pos0=pos0, filter_str="PASS").encode()
    v = la.Vcf.open(caller, text)
    assert v.n_records == len(recs) and v.header()[1]
    # filter: the structs made from the text equal the structs made from the records, and so do lfq_filter_vars' answers
    L = _lib.load()
    hand = np.zeros(len(recs), _lib.FILTER_VAR_DTYPE)
    rr = np.ascontiguousarray(recs, _lib.SNV_RECORD_DTYPE)
    for i in range(len(recs)):
        L.lfq_filter_var_from_snv(rr[i:i + 1].ctypes.data, hand[i:i + 1].ctypes.data)
    got = v.filter_vars()
    assert got.tobytes() == hand.tobytes()
    fails = []
    for arr in (got, hand):
        c = _lib.FilterConf()
        L.lfq_filter_conf_init(C.byref(c))
        L.lfq_filter_conf_defaults(C.byref(c))
        fail = np.zeros(len(arr), np.uint32)
        assert L.lfq_filter_vars(C.byref(c), arr.ctypes.data, len(arr), fail.ctypes.data) == 0
        fails.append(fail)
    assert np.array_equal(fails[0], fails[1])
    # uniq: the variants from the text give what the same variants built by hand give
    u = v.uniq_variants(name, only_unfiltered=True)
    p = vm.parse(text)
    assert u["pos"].tolist() == pos0.tolist() and u["ref"] == [x.ref for x in p.recs] and u["alt"] == [x.alt for x in p.recs]
    a = rs.uniq(u["pos"], [x.decode() for x in u["ref"]], [x.decode() for x in u["alt"]], u["af"], indel_key=u["indel_key"])
    b = rs.uniq(pos0, [x.ref.decode() for x in p.recs], [x.alt.decode() for x in p.recs], hand["af"])
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    v.close()
    rs.close()


def test_nothing_is_launched_that_need_not_be(caller):
    import lofreq_amd as la
    v = la.Vcf.open(caller, b"")
    t = la.last_vcf_times(caller)
    assert t["n_launches"] == 0 and v.n_records == 0 and v.header() == (b"", False)
    assert len(v.filter_vars()) == 0 and v.ign_mask("c1", 10).sum() == 0
    out = la.vcfset(v, op="concat")
    assert (out["text"], out["n_out"]) == (b"", 0) and la.last_vcf_times(caller)["n_launches"] == 0
    one = la.Vcf.open(caller, ve.ONE)
    out = la.vcfset(one, more=[v], op="concat", count_only=True)
    t = la.last_vcf_times(caller)
    assert out["text"] == b"" and out["n_out"] == len(vm.parse(ve.ONE).recs) and t["n_set_launches"] == 1      # the match alone
    out = la.vcfset(one, more=[v], op="concat")
    assert la.last_vcf_times(caller)["n_set_launches"] == 4                 # match, plan, scan, copy
    one.close()
    v.close()
