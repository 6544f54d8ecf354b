"""CPU tests of the BAM-record road (lfq_readset_create_from_bam, lfq_region_add_record): the record encoder of tests/bam_records.py
against its own restatement of the host loop, the ABI of the new entry points, the refusals that need no device, and the region
binding's build.  No compute."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bam_records as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFQ_ERR_INVALID = -1


@pytest.mark.parametrize("name", sorted(br.edge_cases()))
def test_encoder_round_trip(name):
    """what expected_arrays reads out of the encoded bytes is what went in: bases through both tables, qualities, the BI / BD a
    read was given (where the case leaves the aux block to the encoder), descriptors"""
    reads, kw = br.edge_cases()[name]
    recs = br.encode(reads, **kw)
    E = br.expected_arrays(recs)
    assert recs["data_off"][0] == kw.get("first_offset", 0) and recs["data_off"][-1] == len(recs["data"])
    so = E["seq_off"]
    for i, r in enumerate(reads):
        s = slice(so[i], so[i + 1])
        want = br.NT16_INT[np.asarray(r["nib"])] if "nib" in r else np.asarray(r["seq"])
        assert np.array_equal(E["seq"][s], want) and np.array_equal(E["qual"][s], r["qual"]), (name, i)
        assert E["pos"][i] == r["pos0"] and E["mapq"][i] == r["mapq"] and E["rev"][i] == int(r["reverse"])
        assert [(br.OPS[w & 15], w >> 4) for w in E["cig"][E["cig_off"][i]:E["cig_off"][i + 1]].tolist()] == r["cigar"]
        if "aux_raw" not in r:
            for bit, tag in enumerate(("bi", "bd")):
                assert bool(E["flags"][i] >> bit & 1) == (r.get(tag) is not None), (name, i, tag)
                assert np.array_equal(E[tag][s], r[tag] if r.get(tag) is not None else np.full(so[i + 1] - so[i], 33)), (name, i, tag)


def test_the_binding_rules_on_hand_made_aux_blocks():
    C_ = br.edge_cases()
    flags = lambda name: br.expected_arrays(br.encode(*C_[name][:1], **C_[name][1]))["flags"].tolist()
    assert flags("bi_one_shorter_than_l_qseq") == [3, 2, 3]
    assert flags("bi_equal_than_l_qseq") == [3, 3, 3] and flags("bi_longer_than_l_qseq") == [3, 3, 3]
    assert flags("bi_of_type_H_is_ignored") == [2, 3] and flags("bi_of_type_A_is_ignored") == [2, 3]
    assert flags("two_bi_fields_first_too_short") == [0, 3]
    E = br.expected_arrays(br.encode(*C_["two_bi_fields_first_wins"][:1]))
    assert E["flags"].tolist() == [1] and np.array_equal(E["bi"], 33 + (np.arange(10) * 3) % 60)
    E = br.expected_arrays(br.encode(*C_["only_the_last_read_has_bi"][:1]))
    assert E["any_bi"] and not E["any_bd"] and E["flags"].tolist() == [0] * 70 + [1]
    E = br.expected_arrays(br.encode(*C_["all_16_nibble_codes"][:1]))
    assert E["seq"][1:17].tolist() == [5, 0, 1, 6, 2, 7, 8, 9, 3, 10, 11, 12, 13, 14, 15, 4]


def test_the_new_symbols_are_declared_bound_and_exported():
    from lofreq_amd import _lib, pileup
    import lofreq_amd as la
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    assert "int lfq_readset_create_from_bam(lfq_ctx *ctx, const lfq_bam_records *recs, lfq_readset **out);" in hdr
    assert re.search(r"int lfq_readset_fetch_bases\(lfq_ctx \*ctx, lfq_readset \*rs, uint8_t \*seq_out, uint8_t \*qual_out, "
                     r"uint8_t \*bi_out, uint8_t \*bd_out,\s*uint8_t \*tag_flags_out\);", hdr)
    assert "int lfq_last_bam_decode_times(lfq_ctx *ctx, lfq_bam_decode_times *t);" in hdr
    for name in ("lfq_readset_create_from_bam", "lfq_readset_fetch_bases", "lfq_last_bam_decode_times"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    rhdr = open(os.path.join(ROOT, "integration", "lofreq_amd_region.h")).read()
    assert re.search(r"int lfq_region_add_record\(lfq_region \*r, int32_t pos, int flag, int mapq, int l_qname, int n_cigar, "
                     r"int l_qseq,\s*const uint8_t \*data, int l_data\);", rhdr)
    vp = C.c_void_p
    assert L.lfq_readset_create_from_bam.argtypes == [vp, C.POINTER(_lib.BamRecords), C.POINTER(vp)]
    assert L.lfq_readset_fetch_bases.argtypes == [vp] * 7
    assert L.lfq_last_bam_decode_times.argtypes == [vp, C.POINTER(_lib.BamDecodeTimes)]
    assert C.sizeof(_lib.BamRecords) == 11 * 8 and C.sizeof(_lib.BamDecodeTimes) == 7 * 8
    assert callable(pileup.ReadSet.from_bam_records) and callable(pileup.ReadSet.fetch_bases) and callable(la.last_bam_decode_times)
    assert int(re.search(r"#define LFQ_ABI_VERSION (\d+)", hdr).group(1)) == 10 and L.lfq_abi_version() == 10


def _records(recs, **change):
    a = dict(recs, **change)
    rc = C.c_void_p, None
    from lofreq_amd import _lib
    rc = _lib.BamRecords()
    rc.n_reads = a.get("n_reads", len(recs["pos"]))
    for k in ("data", "data_off", "pos", "flag", "mapq", "l_qname", "n_cigar", "l_qseq"):
        setattr(rc, k, None if a[k] is None else a[k].ctypes.data)
    rc.ref = None if a["ref"] is None else C.cast(C.c_char_p(a["ref"]), C.c_void_p)
    rc.ref_len = 0 if a["ref"] is None else len(a["ref"])
    return rc, a                                            # (a keeps the arrays alive)


def test_host_checked_refusals_need_no_device():
    """every case the header lists as checked before a device is touched, with a context handle that is no context: a call that
    went on to the device would not come back with LFQ_ERR_INVALID"""
    from lofreq_amd import _lib
    L = _lib.load()
    recs = br.encode([br.mk(9, 1), br.mk(12, 2), br.mk(5, 3, tags=None)], ref=b"ACGT" * 40)
    bogus = C.create_string_buffer(4096)                    # zeroes where an lfq_ctx would lie: never dereferenced by the checks
    ctx = C.cast(bogus, C.c_void_p)
    out = C.c_void_p(0xdead)
    rc, keep = _records(recs)
    assert L.lfq_readset_create_from_bam(None, C.byref(rc), C.byref(out)) == LFQ_ERR_INVALID and out.value is None
    assert L.lfq_readset_create_from_bam(ctx, None, C.byref(out)) == LFQ_ERR_INVALID
    assert L.lfq_readset_create_from_bam(ctx, C.byref(rc), None) == LFQ_ERR_INVALID
    rc, keep = _records(recs, n_reads=-1)
    assert L.lfq_readset_create_from_bam(ctx, C.byref(rc), C.byref(out)) == LFQ_ERR_INVALID
    for k in ("data", "data_off", "pos", "flag", "mapq", "l_qname", "n_cigar", "l_qseq", "ref"):
        rc, keep = _records(recs, **{k: None})
        out = C.c_void_p(0xdead)
        assert L.lfq_readset_create_from_bam(ctx, C.byref(rc), C.byref(out)) == LFQ_ERR_INVALID, k
        assert out.value is None
    off = recs["data_off"].copy()
    off[1], off[2] = off[2], off[1]
    rc, keep = _records(recs, data_off=off)
    assert L.lfq_readset_create_from_bam(ctx, C.byref(rc), C.byref(out)) == LFQ_ERR_INVALID            # decreasing data_off
    lq = recs["l_qseq"].copy()
    lq[1] = -1
    rc, keep = _records(recs, l_qseq=lq)
    assert L.lfq_readset_create_from_bam(ctx, C.byref(rc), C.byref(out)) == LFQ_ERR_INVALID            # l_qseq < 0
    for k, add in (("l_qseq", 40), ("n_cigar", 30), ("l_qname", 200)):                                # a record shorter than its fields
        a = recs[k].copy()
        a[2] += add
        rc, keep = _records(recs, **{k: a})
        assert L.lfq_readset_create_from_bam(ctx, C.byref(rc), C.byref(out)) == LFQ_ERR_INVALID, k
    # exactly as long as its fields (no aux) passes the check: one byte less does not
    short = br.encode([br.mk(9, 1, tags=None)], ref=b"ACGT" * 40)
    off = short["data_off"].copy()
    off[1] -= 1
    rc, keep = _records(short, data_off=off)
    assert L.lfq_readset_create_from_bam(ctx, C.byref(rc), C.byref(out)) == LFQ_ERR_INVALID
    t = _lib.BamDecodeTimes()
    assert L.lfq_last_bam_decode_times(None, C.byref(t)) == LFQ_ERR_INVALID and L.lfq_last_bam_decode_times(ctx, None) == LFQ_ERR_INVALID
    assert L.lfq_readset_fetch_bases(None, None, None, None, None, None, None) == LFQ_ERR_INVALID


def test_region_binding_still_compiles_with_the_chain_tests_flags(tmp_path):
    lib = str(tmp_path / "liblofreq_amd_region.so")
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "lofreq_amd_region.c"),
                    "-L" + os.path.join(ROOT, "lofreq_amd"), "-llofreq_amd", "-Wl,-rpath," + os.path.join(ROOT, "lofreq_amd"),
                    "-o", lib], check=True, capture_output=True, text=True)
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    assert " T lfq_region_add_record" in syms and " T lfq_region_add_read" in syms
