"""CPU tests of the tag-reuse road: the Python model of the stored-tag decode and the merge rule (tests/tag_reuse_model.py) held to
the 2.1.4 binary through tests/golden/tag_reuse.json, the model's aux walk held to bam_records._aux_get, and the C ABI of the new
entry points without a device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import bam_records as br
import tag_reuse_model as trm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tag_reuse.json")
LFQ_ERR_INVALID = -1
NEW = ("lfq_readset_create_from_bam_tags", "lfq_readset_fetch_stored_tags", "lfq_readset_baq_fill", "lfq_last_baq_fill_stats")


@pytest.fixture(scope="module")
def fx():
    return json.load(open(FIXTURE))


# ---- the model against the binary ---------------------------------------------------------------------------------------------

def test_fixture_is_data_and_small(fx):
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "bam_write.json"))
    assert set(fx) == {"name", "generator", "reference_binary", "seed", "call_args", "genome", "read_fields", "reads", "alnqual",
                       "alnqual_r", "vcf", "vcf_D", "vcf_stripped"}
    shapes = {("I" in r[3], "D" in r[3]) for r in fx["reads"]}
    assert len(shapes) == 4
    for shape in shapes:                # every subset of the three tags on every shape, and strings longer than l_qseq
        subsets = {tuple(sorted(r[6])) for r in fx["reads"] if ("I" in r[3], "D" in r[3]) == shape}
        assert len(subsets) == 8
    assert any(v[1] > 0 for r in fx["reads"] for v in r[6].values())
    a, b, c = fx["vcf"]["vcf"], fx["vcf_D"]["vcf"], fx["vcf_stripped"]["vcf"]
    assert a != b and a != c and b != c
    assert any("INDEL" in l for l in a) and any("INDEL" not in l for l in a)


def test_merge_rule_reproduces_alnqual_without_r(fx):
    """for every record: model(stored = the first fields of the input, computed = what `alnqual -r` wrote) = the first fields
    `alnqual` without -r left -- baq_flag = 1, idaq_flag = 1, the flags of `lofreq call --call-indels`"""
    import golden_util as gu
    reads, recs = trm.fixture_records(fx)
    n_need = n_kept = 0
    for r, rd in enumerate(fx["reads"]):
        l = len(rd[4])
        ff = trm.first_fields(trm.record_aux(recs, r))
        stored = {t.decode(): (ff[t][1][:l] if t in ff else None) for t in trm.TAGS}
        assert {t for t in stored if stored[t] is not None} == set(rd[6])
        computed = dict(zip(("lb", "ai", "ad"), (s.encode() if s is not None else None for s in fx["alnqual_r"][r])))
        assert computed["lb"] is not None and len(computed["lb"]) == l
        hi, hd = trm.has_ins_del(gu.parse_cigar(rd[3]))
        assert (computed["ai"] is not None, computed["ad"] is not None) == (hi, hd)
        out, need = trm.merge_read(stored, computed, hi, hd, want_idaq=True, redo_baq=False)
        got = {t: (s.encode()[:l] if s is not None else None) for t, s in zip(("lb", "ai", "ad"), fx["alnqual"][r])}
        assert out == got, (r, rd[3], sorted(rd[6]))
        n_need += need
        n_kept += any(out[t] is not None and out[t] == stored[t] for t in out)
    assert 0 < n_need < len(fx["reads"]) and n_kept >= 50


def test_need_rule_table():
    """bam_md_ext.c:352-366 by hand"""
    for S in range(8):
        for hi in (False, True):
            for hd in (False, True):
                skip = bool(S & 1) and not (hd and not S & 4) and not (hi and not S & 2)
                assert trm.need_hmm(S, hi, hd, True) == (not skip)
                assert trm.need_hmm(S, hi, hd, False) == (not S & 1)
    assert trm.effective_bits(7, True, True) == 6 and trm.effective_bits(7, False, False) == 1 and trm.effective_bits(7, False, True) == 0


# ---- the stored-tag decode of the model against _aux_get ----------------------------------------------------------------------------

def tagged(l, seed, subset, extra=0, before=(), after=(), bibd="both"):
    """a read of l bases with BI / BD and the lb / ai / ad strings of `subset` (bit 0 / 1 / 2), each l + extra bytes"""
    r = br.mk(l, seed, tags=bibd)
    rng = np.random.default_rng(77 * l + seed)
    aux = b"".join(before)
    for t in ("bi", "bd"):
        if r.get(t) is not None:
            aux += br.aux_field(t.upper(), "Z", r[t].tobytes())
    for k, t in enumerate(("lb", "ai", "ad")):
        if subset >> k & 1:
            aux += br.aux_field(t, "Z", (33 + rng.integers(0, 94, l + extra)).astype(np.uint8).tobytes())
    r["aux_raw"] = aux + b"".join(after)
    return r


def stored_edge_cases():
    """name -> (reads, keyword arguments of bam_records.encode), in the style of bam_records.edge_cases()"""
    chunks = br.source_constant("LFQ_BAM_BASE_CHUNKS")
    aux_reads = br.source_constant("LFQ_BAM_AUX_READS")
    lens = (1, 2, 15, 16, 17, 31, 33)
    many = lambda n: [tagged(lens[i % 7], i, i % 8, extra=(i // 8) % 3, bibd=("both", "bi", "bd", None)[i % 4]) for i in range(n)]
    cases = {}
    for l in lens:
        cases["l_qseq_%d_every_subset" % l] = ([tagged(l, s, s) for s in range(8)], {})
    r = br.mk(10, 13, tags=None)
    z = lambda tag, l, seed: br.aux_field(tag, "Z", (40 + (np.arange(l) * seed) % 50).astype(np.uint8).tobytes())
    r["aux_raw"] = z("lb", 10, 3) + z("ai", 10, 5) + z("lb", 10, 7) + z("ai", 12, 11) + z("ad", 10, 13) + z("ad", 10, 17)
    cases["two_fields_of_a_tag_first_wins"] = ([r, tagged(5, 1, 0)], {})
    every = br.one_of_every_type()
    cases["tags_behind_every_type"] = ([tagged(9 + i, i, 7 - i % 8, before=every) for i in range(8)], {})
    cases["tags_in_front_of_every_type"] = ([tagged(9 + i, i, i % 8, after=every) for i in range(8)], {})
    cases["strings_longer_than_l_qseq"] = ([tagged(l, l, 7, extra=e) for l in (1, 16, 33) for e in (1, 3, 40)], {})
    for o in range(4):
        cases["first_record_at_offset_%d" % o] = (many(9), {"first_offset": o})
    for n in (1, 63, 64, 65, aux_reads + 1):
        cases["%d_reads" % n] = (many(n), {})
    cases["chunks_of_short_reads_that_alternate"] = ([tagged(1 + i % 3, i, (0, 7, 0, 1, 0, 6)[i % 6], bibd=None)
                                                       for i in range(16 * chunks // 2 + 40)], {})
    cases["a_read_longer_than_a_workgroups_tile"] = ([tagged(7, 1, 5), tagged(16 * chunks + 5, 2, 7), tagged(9, 4, 0), tagged(11, 5, 2)], {})
    cases["only_the_last_read_tagged"] = ([tagged(30, i, 0) for i in range(70)] + [tagged(30, 99, 7)], {})
    cases["no_read_tagged"] = ([tagged(20, i, 0, bibd=("both", None)[i % 2]) for i in range(7)], {})
    return cases


def unusable_cases():
    """name -> aux bytes whose FIRST lb field cannot be used (a usable one behind it changes nothing)"""
    l = 21
    good = br.aux_field("lb", "Z", bytes([50]) * l)
    return {"lb_of_type_A": br.aux_field("lb", "A", b"L") + good, "lb_of_type_H": br.aux_field("lb", "H", b"1A" * l) + good,
            "lb_one_byte_short": br.aux_field("lb", "Z", bytes([50]) * (l - 1)) + good}


@pytest.mark.parametrize("name", sorted(stored_edge_cases()))
def test_model_decode_against_aux_get(name):
    reads, kw = stored_edge_cases()[name]
    recs = br.encode(reads, ref=b"ACGT", **kw)
    E = trm.stored_tags(recs)
    off = np.concatenate([[0], np.cumsum(recs["l_qseq"])])
    assert len(E["lb"]) == off[-1]
    for r in range(len(reads)):
        aux, l = trm.record_aux(recs, r), int(recs["l_qseq"][r])
        for k, t in enumerate(trm.TAGS):
            z = br._aux_get(aux, t)
            got = E[t.decode()][off[r]:off[r + 1]].tobytes()
            if z is None:
                assert not E["flags"][r] >> k & 1 and got == b"!" * l
            else:
                assert E["flags"][r] >> k & 1 and got == z[:l] and len(z) >= l
    if name == "no_read_tagged":
        assert not E["flags"].any()
    if name == "two_fields_of_a_tag_first_wins":
        assert E["flags"][0] == 7 and E["lb"][1] == 40 + 3 and E["ai"][1] == 40 + 5 and E["ad"][1] == 40 + 13
    only = trm.stored_tags(recs, trm.READ_LB)
    assert np.array_equal(only["flags"], E["flags"] & 1) and np.array_equal(only["lb"], E["lb"]) and (only["ai"] == 33).all()


@pytest.mark.parametrize("name", sorted(unusable_cases()))
def test_model_refuses_an_unusable_first_field(name):
    bad = br.mk(21, 3, tags=None)
    bad["aux_raw"] = unusable_cases()[name]
    recs = br.encode([br.mk(8, 1), bad, br.mk(13, 2)], ref=b"ACGT")
    with pytest.raises(trm.Unusable):
        trm.stored_tags(recs)
    assert not trm.stored_tags(recs, trm.READ_IDAQ)["flags"].any()      # lb is not looked at


# ---- the C ABI without a device ----------------------------------------------------------------------------------------------------

def test_new_names_are_declared_bound_and_exported():
    import lofreq_amd as la
    from lofreq_amd import _lib, pileup
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes
    assert re.search(r"#define LFQ_BAM_READ_LB\s+1\b", hdr) and re.search(r"#define LFQ_BAM_READ_IDAQ\s+2\b", hdr)
    assert (la.LFQ_BAM_READ_LB, la.LFQ_BAM_READ_IDAQ) == (1, 2)
    for k in ("LFQ_BAM_READ_LB", "LFQ_BAM_READ_IDAQ", "last_baq_fill_stats"):
        assert k in la.__all__ and hasattr(la, k)
    for m in ("fetch_stored_tags", "baq_fill"):
        assert callable(getattr(pileup.ReadSet, m))
    assert "read_tags" in pileup.ReadSet.from_bam_records.__func__.__code__.co_varnames
    region = open(os.path.join(ROOT, "integration", "lofreq_amd_region.h")).read()
    assert re.search(r"\bint lfq_region_set_reuse_tags\(lfq_region \*r, int mode\);", region)


def test_struct_size_and_abi_numbers():
    from lofreq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    assert C.sizeof(_lib.BaqFillStats) == 5 * 8 + 2 * 4 + 2 * 4 == 56
    body = re.search(r"typedef struct lfq_baq_fill_stats \{(.*?)\} lfq_baq_fill_stats;", hdr, re.S).group(1)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    assert names == [f[0] for f in _lib.BaqFillStats._fields_]
    assert _lib.load().lfq_abi_version() == _lib.LFQ_ABI_VERSION == int(re.search(r"#define LFQ_ABI_VERSION (\d+)", hdr).group(1)) == 10


def test_invalid_arguments_without_a_device():
    from lofreq_amd import _lib
    L = _lib.load()
    recs = br.encode([br.mk(8, 1)], ref=b"ACGT")
    rc = _lib.BamRecords()
    rc.n_reads = 1
    for k in ("data", "data_off", "pos", "flag", "mapq", "l_qname", "n_cigar", "l_qseq"):
        setattr(rc, k, recs[k].ctypes.data)
    rc.ref = C.cast(C.c_char_p(b"ACGT"), C.c_void_p)
    rc.ref_len = 4
    out = C.c_void_p(0xdead)
    fake = C.c_void_p(0x1000)           # never dereferenced: every call below is refused on its arguments
    assert L.lfq_readset_create_from_bam_tags(None, C.byref(rc), 1, C.byref(out)) == LFQ_ERR_INVALID and out.value is None
    assert L.lfq_readset_create_from_bam_tags(None, C.byref(rc), 0, C.byref(out)) == LFQ_ERR_INVALID
    assert L.lfq_readset_create_from_bam_tags(fake, None, 3, C.byref(out)) == LFQ_ERR_INVALID
    assert L.lfq_readset_create_from_bam_tags(fake, C.byref(rc), 3, None) == LFQ_ERR_INVALID
    for bits in (4, 8, 1 << 31, 7):
        out = C.c_void_p(0xdead)
        assert L.lfq_readset_create_from_bam_tags(fake, C.byref(rc), bits, C.byref(out)) == LFQ_ERR_INVALID and out.value is None
    assert L.lfq_readset_fetch_stored_tags(None, fake, None, None, None, None) == LFQ_ERR_INVALID
    assert L.lfq_readset_fetch_stored_tags(fake, None, None, None, None, None) == LFQ_ERR_INVALID
    assert L.lfq_readset_baq_fill(None, fake, 1, 1, 0) == LFQ_ERR_INVALID
    assert L.lfq_readset_baq_fill(fake, None, 1, 1, 0) == LFQ_ERR_INVALID
    s = _lib.BaqFillStats()
    assert L.lfq_last_baq_fill_stats(None, C.byref(s)) == LFQ_ERR_INVALID
    assert L.lfq_last_baq_fill_stats(fake, None) == LFQ_ERR_INVALID
