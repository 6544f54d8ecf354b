"""-m gpu: lfq_bgzf_deflate -- bytes cut into BGZF blocks and compressed on the device -- over the table of tests/deflate_edges.py,
byte for byte against the host program lfq_deflate_check.cpp (held to the format by tests/test_deflate_edges.py) and read back by
zlib; at the kernel's blocks-per-workgroup boundaries; with cuts, the end-of-file marker and input that is on the device already;
and lfq_bam_frame_encoded -- the body of a BAM file from the live encode result -- against the bytes htslib wrote and the model of
tests/test_abi_bgzf_deflate.py, alone and chained into the deflate."""
import base64
import ctypes as C
import gzip
import json
import os
import struct
import zlib

import numpy as np
import pytest

import bam_records as br
import bgzf_edges as be
import deflate_edges as de
import golden_util as gu
from test_abi_bgzf_deflate import cigar_words, parse_bam_body, record_bin, reg2bin
from test_bam_write_model import GOLDEN, golden_records
from test_deflate_edges import _compile, run_rows

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

ROWS = {r.name: r for r in de.ROWS}
W = br.source_constant("LFQ_BGZF_DEF_BLOCKS_PER_WG", "lofreq_amd/csrc/lfq_bgzf_deflate.hip")
HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")
LFQ_ERR_INVALID = -1


@pytest.fixture(scope="module")
def host_streams(tmp_path_factory):
    """name -> (block type, stream) as the host program prints them"""
    exe, r = _compile(tmp_path_factory.mktemp("deflate_gpu"), "lfq_deflate_check", [])
    assert r.returncode == 0, r.stderr
    return {row.name: res[:2] for row, res in zip(de.ROWS, run_rows(exe, de.ROWS))}


def _blocks(comp, comp_off):
    return [comp[comp_off[b]:comp_off[b + 1]].tobytes() for b in range(len(comp_off) - 1)]


def _check_block(block, payload):
    """header, BSIZE, stream, CRC-32 and ISIZE of one block; -> the stream"""
    assert block[:16] == HEAD and struct.unpack("<H", block[16:18])[0] == len(block) - 1
    assert struct.unpack("<II", block[-8:]) == (zlib.crc32(payload), len(payload))
    assert zlib.decompress(block, 31) == payload
    return block[18:-8]


@pytest.mark.parametrize("name", [r.name for r in de.ROWS])
def test_every_row_equals_the_host_program(caller, host_streams, name):
    import lofreq_amd as la
    row = ROWS[name]
    comp, comp_off, data_off, btype = la.bgzf_deflate(caller, row.payload)
    want_type, want_stream = host_streams[name]
    assert comp_off.tolist() == [0, len(comp)] and data_off.tolist() == [0, len(row.payload)] and btype.tolist() == [want_type]
    stream = _check_block(comp.tobytes(), row.payload)
    assert stream == want_stream, (name, len(stream), len(want_stream))
    assert (stream[0] >> 1) & 3 == want_type
    if row.cap is not None:
        assert len(stream) <= row.cap
    t = la.last_bgzf_deflate_times(caller)
    assert (t["n_blocks"], t["n_in_bytes"], t["n_out_bytes"], t["n_launches"], t["n_from_device"]) == (1, len(row.payload), len(comp), 2, 0)


@pytest.mark.parametrize("n", [W - 1, W, W + 1, 2 * W + 1, 9])
def test_block_counts_around_the_workgroup(caller, n):
    """every block gets its own bytes and its own place: sizes that put the blocks at every alignment (the grid is one wavefront
    per block, not a persistent one: there is no wrap to test)"""
    import lofreq_amd as la
    sizes = [1, 4093, 65280, 17, 3000, 2, 777, 50001, 64][:n]
    assert len(sizes) == n >= 1
    pays = [be._payload(s, 100 + i) for i, s in enumerate(sizes)]
    data = b"".join(pays)
    cuts = np.cumsum(sizes)[:-1]
    comp, comp_off, data_off, btype = la.bgzf_deflate(caller, data, cuts=cuts)
    assert data_off.tolist() == [0] + np.cumsum(sizes).tolist() and len(btype) == n and comp_off[0] == 0 and comp_off[-1] == len(comp)
    for blk, p, bt in zip(_blocks(comp, comp_off), pays, btype.tolist()):
        assert (_check_block(blk, p)[0] >> 1) & 3 == bt
    assert gzip.decompress(comp.tobytes()) == data
    if n == 9:
        assert set((comp_off[:-1] % 4).tolist()) == {0, 1, 2, 3}, comp_off.tolist()


def test_default_cuts_every_65280_bytes(caller):
    import lofreq_amd as la
    data = be._payload(2 * de.N + 5, 3)
    comp, comp_off, data_off, btype = la.bgzf_deflate(caller, data)
    assert data_off.tolist() == [0, de.N, 2 * de.N, 2 * de.N + 5]
    assert gzip.decompress(comp.tobytes()) == data
    for b, blk in enumerate(_blocks(comp, comp_off)):
        _check_block(blk, data[data_off[b]:data_off[b + 1]])


def test_custom_cuts_and_the_end_of_file_marker(caller):
    """a 1-byte piece and a 65280-byte piece next to each other; the marker behind the blocks, not counted"""
    import lofreq_amd as la
    data = be._payload(700 + 1 + de.N + 33, 4)
    cuts = [700, 701, 701 + de.N]
    comp, comp_off, data_off, btype = la.bgzf_deflate(caller, data, cuts=cuts, eof=True)
    assert data_off.tolist() == [0] + cuts + [len(data)] and len(btype) == 4
    assert comp[-28:].tobytes() == be.EOF_BLOCK and comp_off[-1] == len(comp) - 28
    for b, blk in enumerate(_blocks(comp, comp_off)):
        _check_block(blk, data[data_off[b]:data_off[b + 1]])
    assert gzip.decompress(comp.tobytes()) == data
    plain = la.bgzf_deflate(caller, data, cuts=cuts)[0]
    assert plain.tobytes() == comp[:-28].tobytes()
    data_in, off, st = la.bgzf_inflate(caller, comp)                # and the project's own way in reads it back
    assert data_in.tobytes() == data and not st.any() and off.tolist() == data_off.tolist() + [len(data)]


def test_empty_input_launches_nothing(caller):
    import lofreq_amd as la
    la.bgzf_deflate(caller, b"something")
    assert la.last_bgzf_deflate_times(caller)["n_launches"] == 2
    comp, comp_off, data_off, btype = la.bgzf_deflate(caller, b"")
    assert len(comp) == 0 and comp_off.tolist() == [0] and data_off.tolist() == [0] and len(btype) == 0
    t = la.last_bgzf_deflate_times(caller)
    assert t["n_launches"] == 0 and t["n_blocks"] == 0 and t["n_out_bytes"] == 0
    comp, comp_off, _, _ = la.bgzf_deflate(caller, b"", eof=True)
    assert comp.tobytes() == be.EOF_BLOCK and comp_off.tolist() == [0]
    comp = la.bgzf_deflate(caller, b"still usable")[0]              # the context stays usable
    assert gzip.decompress(comp.tobytes()) == b"still usable"


def test_input_inside_the_inflate_result_stays_on_the_device(caller):
    """bgzf_inflate of zlib-written blocks, then bgzf_deflate of a slice of its result by pointer"""
    import lofreq_amd as la
    from lofreq_amd import _lib
    from lofreq_amd.pileup import bgzf_deflated_arrays
    L = _lib.load()
    payload = be._payload(150000, 9)
    zcomp = np.frombuffer(be.bgzf_blocks(payload, [60001, 120002]), np.uint8).copy()
    res = C.POINTER(_lib.BgzfResult)()
    assert L.lfq_bgzf_inflate(caller.h, zcomp.ctypes.data, len(zcomp), C.byref(res)) == 0
    assert res.contents.n_bytes == len(payload)
    a, b = 1237, 1237 + 70003                                       # an odd start, more than one block
    out = C.POINTER(_lib.BgzfDeflated)()
    assert L.lfq_bgzf_deflate(caller.h, res.contents.data + a, b - a, None, 0, 0, C.byref(out)) == 0
    comp, comp_off, data_off, btype = bgzf_deflated_arrays(out.contents)
    t = la.last_bgzf_deflate_times(caller)
    assert t["n_from_device"] == 1 and t["n_blocks"] == 2 and t["n_in_bytes"] == b - a
    assert gzip.decompress(comp.tobytes()) == payload[a:b]
    again = la.bgzf_deflate(caller, payload[a:b])                   # the same bytes handed over from elsewhere
    assert la.last_bgzf_deflate_times(caller)["n_from_device"] == 0
    assert again[0].tobytes() == comp.tobytes() and again[1].tolist() == comp_off.tolist() and again[3].tolist() == btype.tolist()


# ---- lfq_bam_frame_encoded -----------------------------------------------------------------------------------------------------------

def _from(la, caller, recs):
    return la.ReadSet.from_bam_records(caller, recs["data"], recs["data_off"], recs["pos"], recs["flag"], recs["mapq"],
                                       recs["l_qname"], recs["n_cigar"], recs["l_qseq"], recs["ref"])


def _records_of(parsed, ref):
    col = lambda k, dt: np.asarray([r[k] for r in parsed], dt)
    return {"data": np.frombuffer(b"".join(r["data"] for r in parsed), np.uint8).copy(),
            "data_off": np.concatenate([[0], np.cumsum([len(r["data"]) for r in parsed])]).astype(np.int64),
            "pos": col("pos", np.int32), "flag": col("flag", np.uint16), "mapq": col("mapq", np.uint8),
            "l_qname": col("l_qname", np.uint16), "n_cigar": col("n_cigar", np.uint32), "l_qseq": col("l_qseq", np.int32), "ref": ref}


def _cores(recs, seed=0):
    """a 32-byte core per record of a records dict: refID 0, a bin that is not the record's, mate fields that differ per record"""
    return b"".join(struct.pack("<iiBBHHHiiii", 0, int(recs["pos"][i]), int(recs["l_qname"][i]), int(recs["mapq"][i]), 0xdead,
                                int(recs["n_cigar"][i]), int(recs["flag"][i]), int(recs["l_qseq"][i]), i % 3 - 1, 1000 + 7 * i + seed,
                                -50 - i) for i in range(len(recs["pos"])))


def _check_framed(body, rec_off, enc, cores):
    """every record of the body: block_size, core' = the core of record src[j] with pos, n_cigar and bin replaced, the bytes"""
    body = bytes(body)
    assert rec_off[0] == 0 and rec_off[-1] == len(body) and len(rec_off) == len(enc["pos"]) + 1
    bins = []
    for j, s in enumerate(enc["src"].tolist()):
        o = int(rec_off[j])
        rec = bytes(enc["data"][enc["data_off"][j]:enc["data_off"][j + 1]])
        assert struct.unpack_from("<i", body, o)[0] == 32 + len(rec) and rec_off[j + 1] - o == 36 + len(rec)
        assert body[o + 36:rec_off[j + 1]] == rec, j
        core, orig = body[o + 4:o + 36], cores[32 * s:32 * s + 32]
        lq, nc = int(enc["l_qname"][j]), int(enc["n_cigar"][j])
        words = np.frombuffer(rec[lq:lq + 4 * nc], "<u4")
        want_bin = record_bin(int(enc["pos"][j]), int(enc["flag"][j]), words)
        assert struct.unpack_from("<i", core, 4)[0] == enc["pos"][j] and struct.unpack_from("<H", core, 12)[0] == nc
        assert struct.unpack_from("<H", core, 10)[0] == want_bin, (j, want_bin)
        assert core[:4] == orig[:4] and core[8:10] == orig[8:10] and core[14:] == orig[14:], j    # every other byte is the caller's
        bins.append(want_bin)
    return bins


def test_frame_gives_back_the_body_htslib_wrote(caller):
    """the records of a BAM the 2.1.4 binary wrote, through decode and encode, framed with the file's own cores whose bin is
    overwritten: the file's inflated bytes from the first record on"""
    import lofreq_amd as la
    fx = json.load(open(os.path.join(gu.GOLDEN_DIR, "bgzf_binary.json")))
    inflated = base64.b64decode(fx["inflated_base64"])
    first, parsed, l_ref = parse_bam_body(inflated)
    recs = _records_of(parsed, b"A" * max(l_ref, max(r["pos"] for r in parsed) + 1000))
    rs = _from(la, caller, recs)
    enc = rs.encode_bam(recs, None, la.LFQ_BAM_PUT_ALIGNMENT)
    cores = b"".join(r["core"][:10] + b"\0\0" + r["core"][12:] for r in parsed)
    body, rec_off = la.bam_frame_encoded(caller, cores)
    assert body.tobytes() == inflated[first:]
    assert rec_off.tolist() == [r["off"] - first for r in parsed] + [len(inflated) - first]
    rs.close()


def test_frame_after_viterbi_in_the_new_order(caller):
    import lofreq_amd as la
    import bam_write_model as wm
    fx = json.load(open(GOLDEN))
    recs = golden_records(fx["input"], fx["genome"].encode())
    rs = _from(la, caller, recs)
    new, _, order = rs.viterbi(-1)
    enc = new.encode_bam(recs, order, wm.VITERBI)
    assert not np.array_equal(order, np.arange(len(order)))
    cores = _cores(recs)
    body, rec_off = la.bam_frame_encoded(caller, cores)
    _check_framed(body, rec_off, enc, cores)
    rs.close()
    new.close()


def test_frame_bin_edge_cases_and_refusals(caller):
    import lofreq_amd as la
    from lofreq_amd import _lib
    import bam_write_model as wm
    L = _lib.load()
    ref = b"ACGTTGCAAGGCTTAACCGGATCGATTACAGGCATCGAGCTA" * 400
    reads = [dict(br.mk(50, 1, pos0=-1, tags=None), flag_other=4),                          # unplaced: bin 4680
             dict(br.mk(20, 2, pos0=100, tags=None), cigar=[("S", 20)]),                      # no reference bases
             dict(br.mk(20, 3, pos0=300, tags=None), cigar=[("S", 3), ("I", 17)]),
             br.mk(20, 4, pos0=16380, tags=None),                                             # across a 16 kb bin edge
             br.mk(33, 5, pos0=16384, tags="both")]
    recs = br.encode(reads, ref=ref)
    rs = _from(la, caller, recs)
    enc = rs.encode_bam(recs, None, wm.DROP_ALN_TAGS)
    cores = _cores(recs, 5)
    body, rec_off = la.bam_frame_encoded(caller, cores)
    bins = _check_framed(body, rec_off, enc, cores)
    assert bins == [4680, reg2bin(100, 101), reg2bin(300, 301), 585, 4682]
    # refusals: the context's result is left as it was
    fr = C.POINTER(_lib.BamFramed)()
    arr = np.frombuffer(cores, np.uint8).copy()
    assert L.lfq_bam_frame_encoded(caller.h, arr.ctypes.data, len(reads) - 1, C.byref(fr)) == LFQ_ERR_INVALID   # n_cores <= an index
    for at, what in ((8, "l_read_name"), (16, "l_seq")):
        bad = arr.copy()
        bad[32 * 3 + at] ^= 1
        assert L.lfq_bam_frame_encoded(caller.h, bad.ctypes.data, len(reads), C.byref(fr)) == LFQ_ERR_INVALID, what
    assert not fr
    again, _ = la.bam_frame_encoded(caller, cores)
    assert again.tobytes() == body.tobytes()
    rs.close()
    # no live encode result: a context that has not encoded
    other = la.SnvCaller(0)
    assert L.lfq_bam_frame_encoded(other.h, arr.ctypes.data, len(reads), C.byref(fr)) == LFQ_ERR_INVALID
    other.close()


def test_empty_encode_frames_to_an_empty_body(caller):
    import lofreq_amd as la
    import bam_write_model as wm
    recs = br.encode([], ref=b"ACGT" * 10)
    rs = _from(la, caller, recs)
    enc = rs.encode_bam(recs, None, wm.DROP_ALN_TAGS)
    assert len(enc["pos"]) == 0
    body, rec_off = la.bam_frame_encoded(caller, b"")
    assert len(body) == 0 and rec_off.tolist() == [0]
    rs.close()


def test_chain_encode_frame_deflate_is_a_bam(caller):
    """viterbi -> encode -> frame -> deflate of the framed body by pointer, behind a header compressed by the same call: gzip reads
    the file back and its records are the ones the encode returned"""
    import lofreq_amd as la
    import bam_write_model as wm
    from lofreq_amd import _lib
    from lofreq_amd.pileup import bgzf_deflated_arrays
    L = _lib.load()
    fx = json.load(open(GOLDEN))
    genome = fx["genome"].encode()
    recs = golden_records(fx["input"], genome)
    rs = _from(la, caller, recs)
    new, _, order = rs.viterbi(-1)
    enc = new.encode_bam(recs, order, wm.VITERBI)
    text = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:%d\n" % len(genome)
    header = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<ii", 1, 5) + b"chr1\0" + struct.pack("<i", len(genome))
    head_blocks = la.bgzf_deflate(caller, header)[0]
    cores = np.frombuffer(_cores(recs), np.uint8).copy()
    fr = C.POINTER(_lib.BamFramed)()
    assert L.lfq_bam_frame_encoded(caller.h, cores.ctypes.data, len(recs["pos"]), C.byref(fr)) == 0
    n, n_bytes = int(fr.contents.n_reads), int(fr.contents.n_bytes)
    rec_off = np.ctypeslib.as_array(C.cast(fr.contents.rec_off, C.POINTER(C.c_int64)), (n + 1,)).copy()
    cuts = rec_off[5:-1:5].copy()                                   # no record is split across blocks
    out = C.POINTER(_lib.BgzfDeflated)()
    assert L.lfq_bgzf_deflate(caller.h, fr.contents.data, n_bytes, cuts.ctypes.data, len(cuts), _lib.LFQ_BGZF_PUT_EOF, C.byref(out)) == 0
    comp, comp_off, data_off, btype = bgzf_deflated_arrays(out.contents)
    t = la.last_bgzf_deflate_times(caller)
    assert t["n_from_device"] == 1 and t["n_blocks"] == len(cuts) + 1 and data_off.tolist() == [0] + cuts.tolist() + [n_bytes]
    assert comp[-28:].tobytes() == be.EOF_BLOCK
    # (make_bamwrite_golden.parse_bam's walk, on bytes instead of a path)
    data = gzip.decompress(head_blocks.tobytes() + comp.tobytes())
    first, parsed, l_ref = parse_bam_body(data)
    assert first == len(header) and l_ref == len(genome) and len(parsed) == n == len(enc["pos"])
    for j, r in enumerate(parsed):
        assert r["data"] == bytes(enc["data"][enc["data_off"][j]:enc["data_off"][j + 1]]), j
        assert (r["pos"], r["n_cigar"], r["flag"], r["mapq"], r["l_qname"], r["l_qseq"]) == tuple(
            int(enc[k][j]) for k in ("pos", "n_cigar", "flag", "mapq", "l_qname", "l_qseq")), j
        assert r["bin"] == record_bin(r["pos"], r["flag"], cigar_words(r))
        assert r["off"] - first == rec_off[j]
    rs.close()
    new.close()
