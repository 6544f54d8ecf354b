"""-m gpu: lfq_bgzf_inflate -- BGZF blocks inflated and CRC-checked on the device -- over the table of tests/bgzf_edges.py (held to
zlib by tests/test_bgzf_edges.py), on a BAM the 2.1.4 binary wrote, at the kernel's blocks-per-workgroup boundaries, and chained
into the BAM decode (ReadSet.from_bgzf) against ReadSet.from_bam_records on the kept records."""
import base64
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

import bam_records as br
import bgzf_edges as be
import golden_util as gu

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

ROWS = {r.name: r for r in be.ROWS if r.frameable}
GOOD_A, GOOD_B = b"in front of the row " * 7, bytes(range(256)) * 3
W = br.source_constant("LFQ_BGZF_BLOCKS_PER_WG", "lofreq_amd/csrc/lfq_bgzf.hip")
ST_MALFORMED, ST_TRUNCATED, ST_OVERRUN, ST_DISTANCE, ST_SIZE, ST_CRC = 1, 2, 3, 4, 5, 6


def _good(p):
    return be.bgzf_block(be.deflate(p), p)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_every_row_between_two_good_blocks(caller, name):
    import lofreq_amd as la
    row = ROWS[name]
    comp = _good(GOOD_A) + be.frame(row) + _good(GOOD_B)
    if row.verdict == "ok":
        data, off, st = la.bgzf_inflate(caller, comp)
        assert st.tolist() == [0, 0, 0] and off.tolist() == list(np.cumsum([0, len(GOOD_A), len(row.payload), len(GOOD_B)]))
        assert data.tobytes() == GOOD_A + row.payload + GOOD_B
        t = la.last_bgzf_times(caller)
        assert (t["n_blocks"], t["n_in_bytes"], t["n_out_bytes"], t["n_launches"]) == (3, len(comp), len(data), 1)
        return
    with pytest.raises(la.BgzfError) as e:
        la.bgzf_inflate(caller, comp)
    st, off, data = e.value.status, e.value.data_off, e.value.data.tobytes()
    assert st[0] == 0 and st[2] == 0 and st[1] != 0, st
    if row.verdict == "deflate":
        assert st[1] in (ST_MALFORMED, ST_TRUNCATED, ST_DISTANCE), (name, st)
    elif row.isize is None:
        assert st[1] == ST_CRC
    else:
        assert st[1] == (ST_OVERRUN if row.isize < len(row.payload) else ST_SIZE), (name, st)
    assert data[off[0]:off[1]] == GOOD_A and data[off[2]:off[3]] == GOOD_B      # the other blocks of the call are intact
    data, _, st = la.bgzf_inflate(caller, _good(GOOD_B))                        # and the context stays usable
    assert data.tobytes() == GOOD_B and st.tolist() == [0]


def test_framing_the_host_refuses(caller):
    import lofreq_amd as la
    before = la.bgzf_inflate(caller, _good(GOOD_A))[0].tobytes()
    for name, comp in sorted(be.FRAMING_BAD.items()):
        with pytest.raises(RuntimeError) as e:
            la.bgzf_inflate(caller, comp)
        assert not isinstance(e.value, la.BgzfError), name
    data, off, st = la.bgzf_inflate(caller, be.EXTRA_SUBFIELD_BLOCK + be.EOF_BLOCK)
    assert data.tobytes() == be.EXTRA_SUBFIELD_PAYLOAD and off.tolist() == [0, len(data), len(data)] and st.tolist() == [0, 0]
    assert before == GOOD_A


def test_empty_input_launches_nothing(caller):
    import lofreq_amd as la
    la.bgzf_inflate(caller, _good(GOOD_A))
    assert la.last_bgzf_times(caller)["n_launches"] == 1
    data, off, st = la.bgzf_inflate(caller, b"")
    assert len(data) == 0 and off.tolist() == [0] and len(st) == 0
    t = la.last_bgzf_times(caller)
    assert t["n_launches"] == 0 and t["n_blocks"] == 0
    data, off, st = la.bgzf_inflate(caller, be.EOF_BLOCK)                       # the end-of-file marker is an ordinary block
    assert len(data) == 0 and off.tolist() == [0, 0] and st.tolist() == [0]


def test_a_bam_the_reference_binary_wrote(caller):
    import lofreq_amd as la
    fx = json.load(open(os.path.join(gu.GOLDEN_DIR, "bgzf_binary.json")))
    bam, want = base64.b64decode(fx["bam_base64"]), base64.b64decode(fx["inflated_base64"])
    assert zlib.crc32(want) == fx["inflated_crc32"]
    data, off, st = la.bgzf_inflate(caller, bam)
    assert not st.any() and data.tobytes() == want and off[-1] == len(want)
    assert want[:4] == b"BAM\1"


@pytest.mark.parametrize("n", [W - 1, W, W + 1, 2 * W + 1])
def test_block_counts_around_the_workgroup(caller, n):
    """every block gets its own bytes: mixed sizes, odd output offsets, the end-of-file marker in the middle"""
    import lofreq_amd as la
    sizes = ([1, 4093, 0, 65280, 17, 3000, 65536, 2] * (n // 8 + 1))[:n]
    assert len(sizes) == n >= 1
    pays = [None if s == 0 else be._payload(s, 100 + i) for i, s in enumerate(sizes)]
    comp = b"".join(be.EOF_BLOCK if p is None else _good(p) for p in pays)
    data, off, st = la.bgzf_inflate(caller, comp)
    assert not st.any() and off.tolist() == list(np.cumsum([0] + sizes))
    for i, p in enumerate(pays):
        assert data[off[i]:off[i + 1]].tobytes() == (p or b""), i


# ---- chained into the decode -------------------------------------------------------------------------------------------------------

def _chain_reads():
    import lofreq_amd as la
    fx = json.load(open(gu.chain_fixtures()[0]))
    reads = []
    for i, r in enumerate(fx["reads"]):
        d = {"pos0": r[0], "cigar": gu.parse_cigar(r[3]), "seq": la.encode_seq(r[4]), "qual": np.array([ord(c) - 33 for c in r[5]], np.uint8),
             "mapq": r[2], "reverse": bool(r[1] & 16), "name": "read%d" % i}
        if i % 3 == 0:                              # a stored lb string for lfq_readset_create_from_bam_tags to find
            d["aux_raw"] = br.aux_field("lb", "Z", bytes(40 + (j % 20) for j in range(len(d["qual"]))))
        reads.append(d)
    return fx, reads


def test_from_bgzf_equals_from_bam_records_on_the_kept_records(caller):
    import lofreq_amd as la
    from test_gpu_readset_viterbi import _cols_equal
    fx, reads = _chain_reads()
    ref = fx["genome"].encode()
    end = max(r["pos0"] for r in reads) - 5         # the reads that start at or behind it are out of the region
    opts = dict(tid=0, beg=0, end=end, min_mq=5, max_mq=255, no_orphan=True)
    items = []
    for i, r in enumerate(reads):
        items.append((r, 0))
        if i % 7 == 0:
            items.append((dict(r, flag_other=4, name="unmapped"), 0))
        if i % 11 == 0:
            items.append((dict(r, flag_other=1024, name="dup"), 0))
        if i % 13 == 0:
            items.append((dict(r, mapq=3, name="lowmq"), 0))
        if i % 17 == 0:
            items.append((dict(r, flag_other=1, name="orphan"), 0))
        if i % 19 == 0:
            items.append((dict(r, name="elsewhere"), 1))
    header = b"BAM\1" + b"h" * 123                  # `first` points behind whatever header the caller has parsed
    payload = header + b"".join(be.bam_record(r, tid) for r, tid in items)
    comp = be.bgzf_blocks(payload, range(997, len(payload), 997)) + be.EOF_BLOCK   # records straddle the block boundaries
    kept = [r for r, tid in items if tid == 0 and not (r.get("flag_other", 0) & (4 | 1024 | 1)) and r["mapq"] >= 5 and r["pos0"] < end]
    assert 0 < len(kept) < len(reads) < len(items)
    rs = la.ReadSet.from_bgzf(caller, comp, len(header), ref, read_tags=la.LFQ_BAM_READ_LB, **opts)
    t = la.last_bgzf_times(caller)
    assert t["n_decodes_from_device"] == 1 and t["n_out_bytes"] == len(payload) and rs.n_consumed == len(payload)
    assert rs.n == len(kept)
    recs = br.encode(kept, ref=ref)
    want = la.ReadSet.from_bam_records(caller, recs["data"], recs["data_off"], recs["pos"], recs["flag"], recs["mapq"],
                                       recs["l_qname"], recs["n_cigar"], recs["l_qseq"], ref, read_tags=la.LFQ_BAM_READ_LB)
    assert la.last_bgzf_times(caller)["n_decodes_from_device"] == 1            # (records from elsewhere: nothing changes)
    assert np.array_equal(rs.seq_off, want.seq_off)
    for a, b in zip(rs.fetch_bases(), want.fetch_bases()):
        assert np.array_equal(a, b)
    got_st, want_st = rs.fetch_stored_tags(), want.fetch_stored_tags()
    assert want_st[3].any() and not want_st[3].all()
    for a, b in zip(got_st, want_st):
        assert np.array_equal(a, b)
    a, pa = rs.pileup_indels(0, len(ref))           # positions, CIGARs, mapq and strand: through the indel pileup
    b, pb = want.pileup_indels(0, len(ref))
    assert np.array_equal(pa, pb) and a.ncols > 50
    _cols_equal(a, b)
    rs.close()
    want.close()


def test_any_decode_of_records_inside_the_result_stays_on_the_device(caller):
    """lfq_readset_create_from_bam with `data` pointing into lfq_bgzf_result.data: a device-to-device copy, counted"""
    import lofreq_amd as la
    from lofreq_amd import _lib
    L = _lib.load()
    ref = ("ACGTTGCAAGGCTTAACCGGATCGATTACAGGCATCGAGCTA" * 12).encode()
    r = br.mk(33, 5, pos0=10)
    lq, nc, ls, body = br.record_fields(r)
    payload = b"x" * 301 + body + b"y" * 77
    comp = np.frombuffer(be.bgzf_blocks(payload, [150, 320]), np.uint8).copy()
    res = C.POINTER(_lib.BgzfResult)()
    assert L.lfq_bgzf_inflate(caller.h, comp.ctypes.data, len(comp), C.byref(res)) == 0
    assert res.contents.n_bytes == len(payload)
    arr = {"data_off": np.array([301, 301 + len(body)], np.int64), "pos": np.array([10], np.int32), "flag": np.array([16 if r["reverse"] else 0], np.uint16),
           "mapq": np.array([r["mapq"]], np.uint8), "l_qname": np.array([lq], np.uint16), "n_cigar": np.array([nc], np.uint32),
           "l_qseq": np.array([ls], np.int32)}
    rc = _lib.BamRecords()
    rc.n_reads = 1
    rc.data = res.contents.data
    for k, v in arr.items():
        setattr(rc, k, v.ctypes.data)
    rc.ref = C.cast(C.c_char_p(ref), C.c_void_p)
    rc.ref_len = len(ref)
    h = C.c_void_p()
    assert L.lfq_readset_create_from_bam(caller.h, C.byref(rc), C.byref(h)) == 0
    assert la.last_bgzf_times(caller)["n_decodes_from_device"] == 1
    seq, qual = np.zeros(ls, np.uint8), np.zeros(ls, np.uint8)
    assert L.lfq_readset_fetch_bases(caller.h, h, seq.ctypes.data, qual.ctypes.data, None, None, None) == 0
    assert np.array_equal(seq, r["seq"]) and np.array_equal(qual, r["qual"])
    L.lfq_readset_destroy(h)


# ---- the region binding fed with compressed blocks ------------------------------------------------------------------------------------

def _run_regions_bgzf(caller, lib, reads, ref, regions, conf, call_indels, mix=None):
    """test_gpu_readset_from_bam.py::_run_regions with every region fed by lfq_region_add_bgzf: ALL the reads (plus reads the scan
    must drop) as a BAM stream with a header in front, compressed in two chunks whose blocks cut through records; the region's
    own [beg, end) picks its reads.  mix: also call that other feed function -> its return code"""
    from test_gpu_chain import _RegionOpts
    P = C.CDLL(lib)
    lines = []
    EMIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)
    cb = EMIT(lambda user, s: lines.append(s.decode().rstrip("\n")))
    o = _RegionOpts()
    P.lfq_region_opts_init(C.byref(o))
    o.use_idaq = o.call_indels = 1 if call_indels else 0
    h = C.c_void_p()
    P.lfq_region_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, EMIT, C.c_void_p]
    assert P.lfq_region_open(C.byref(h), caller.h, C.byref(conf.c), C.byref(o), cb, None) == 0
    P.lfq_region_begin.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int64]
    P.lfq_region_add_bgzf.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_int64, C.c_int64, C.c_int64]
    P.lfq_region_add_record.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
    P.lfq_region_end.argtypes = [C.c_void_p]
    P.lfq_region_close.argtypes = [C.c_void_p, C.c_void_p]
    header = b"BAM\1" + b"t" * 77
    recs = []
    for i, r in enumerate(reads):
        recs.append(be.bam_record(dict(r, name="read%d" % i), 3))
        if i % 9 == 0:
            recs.append(be.bam_record(dict(r, name="dup%d" % i, flag_other=1024), 3))
        if i % 10 == 0:
            recs.append(be.bam_record(dict(r, name="other%d" % i), 2))
    half = len(recs) // 2
    parts = [header + b"".join(recs[:half]), b"".join(recs[half:])]
    chunks = [be.bgzf_blocks(p, range(1501, len(p), 1501)) for p in parts]
    mixed_rc = None
    for beg, end in regions:
        assert P.lfq_region_begin(h, b"chr1", ref, len(ref), beg, end) == 0
        assert P.lfq_region_add_bgzf(h, 3, chunks[0], len(chunks[0]), len(header), -1) == 0
        assert P.lfq_region_add_bgzf(h, 3, chunks[1] + be.EOF_BLOCK, len(chunks[1]) + 28, 0, -1) == 0
        if mix == "record":
            lq, nc, ls, data = br.record_fields(reads[0])
            mixed_rc = P.lfq_region_add_record(h, reads[0]["pos0"], 0, 60, lq, nc, ls, data, len(data))
        assert P.lfq_region_end(h) == 0
    wo = C.c_int64(-1)
    assert P.lfq_region_close(h, C.byref(wo)) == 0
    return lines, wo.value, mixed_rc


@pytest.mark.parametrize("n_regions", [1, 3])
def test_region_binding_fed_with_bgzf_equals_the_record_road(caller, tmp_path, n_regions):
    import lofreq_amd as la
    from test_gpu_chain import _build_region_lib, _epilogue
    from test_gpu_readset_from_bam import _run_regions
    lib = _build_region_lib(tmp_path)
    # the SNV fixture and the indel fixture the 2.1.4 binary wrote
    fx = json.load(open(gu.chain_fixtures()[0]))
    reads = [{"pos0": r[0], "cigar": gu.parse_cigar(r[3]), "seq": la.encode_seq(r[4]),
              "qual": np.array([ord(c) - 33 for c in r[5]], np.uint8), "mapq": r[2], "reverse": bool(r[1] & 16)} for r in fx["reads"]]
    fxi, reads_i = gu.load_plpindel(gu.plpindel_fixtures()[0], with_alnqual_tags=False)
    for ref, rds, kw_args, indels, want in ((fx["genome"].encode(), reads, fx["call_args"], False, fx["vcf"]),
                                            (fxi["genome"].encode(), reads_i, fxi["call_args"], True, fxi["all"]["vcf"])):
        kw, ndf = gu.conf_kwargs(kw_args)
        n = len(ref)
        regions = [(0, n)] if n_regions == 1 else [(0, n // 3), (n // 3, n // 3 + 37), (n // 3 + 37, n)]
        conf_a, conf_b = la.VarcallConf(**kw), la.VarcallConf(**kw)
        lines_a, _, wo_a, _ = _run_regions(caller, lib, rds, ref, regions, conf_a, "record", call_indels=indels)
        lines_b, wo_b, _ = _run_regions_bgzf(caller, lib, rds, ref, regions, conf_b, indels)
        assert lines_b == lines_a and wo_b == wo_a and len(lines_a) > 0
        for k in ("num_snv_tests", "num_indel_tests", "bonf_subst", "bonf_indel"):
            assert getattr(conf_a, k) == getattr(conf_b, k), k
        vcf = _epilogue(la, lines_b, conf_b)
        if indels or ndf:
            assert vcf == want
        else:
            assert [l for l in vcf if l in set(want)] == want


def test_region_binding_refuses_mixed_feeds(caller, tmp_path):
    import lofreq_amd as la
    from test_gpu_chain import _build_region_lib
    lib = _build_region_lib(tmp_path)
    fx = json.load(open(gu.chain_fixtures()[0]))
    reads = [{"pos0": r[0], "cigar": gu.parse_cigar(r[3]), "seq": la.encode_seq(r[4]),
              "qual": np.array([ord(c) - 33 for c in r[5]], np.uint8), "mapq": r[2], "reverse": bool(r[1] & 16)} for r in fx["reads"]]
    ref = fx["genome"].encode()
    kw, _ = gu.conf_kwargs(fx["call_args"])
    _, _, mixed = _run_regions_bgzf(caller, lib, reads, ref, [(0, len(ref))], la.VarcallConf(**kw), False, mix="record")
    assert mixed == -1
