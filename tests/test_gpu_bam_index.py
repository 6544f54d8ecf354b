"""-m gpu: lfq_bam_index_build -- the .bai of a BAM built on the device -- over the table of tests/bai_edges.py against the model
of tests/bai_model.py (bins, chunks, linear index, metadata, n_no_coor, or the refusal and its record); on both BAMs of
tests/golden/bai_binary.json against the .bai the reference's 2.1.4 binary wrote, from host memory and from the resident result of
lfq_bgzf_inflate; at the end of the writing chain encode -> frame -> cuts -> deflate -> index on the framed body by pointer; and
back again: the chunks a query names, inflated and scanned by lfq_readset_create_from_bgzf, hold exactly the region's records."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import bai_edges as be
import bai_model as bm
import bgzf_edges as bz
from test_abi_bam_index import content
from test_bai_model import KINDS, load
from test_bam_write_model import GOLDEN, golden_records

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

ROWS = {r.name: r for r in be.ROWS}
LOFREQ = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "bin", "lofreq")


def _build(la, caller, row):
    return la.bam_index_build(caller, row.body, row.rec_off, row.data_off, row.comp_off, row.file_off, row.n_ref)


@pytest.mark.parametrize("name", [r.name for r in be.ROWS])
def test_every_row_equals_the_model(caller, name):
    import lofreq_amd as la
    row = ROWS[name]
    want = be.expected(row)
    n_recs = len(row.rec_off) - 1
    if isinstance(want, int):
        assert want == row.error
        with pytest.raises(la.BamIndexError) as e:
            _build(la, caller, row)
        assert e.value.record == want, (name, e.value.record)
        if want >= 0:
            t = la.last_bam_index_times(caller)
            assert (t["first_bad_record"], t["n_launches"], t["n_recs"]) == (want, 1, n_recs)
        return
    idx = _build(la, caller, row)
    got = content(idx)
    for t, (g, w) in enumerate(zip(got["refs"], want["refs"])):
        assert g["bins"] == w["bins"], (name, t)
        assert g["linear"] == w["linear"], (name, t)
        assert g["meta"] == w["meta"], (name, t)
    assert got == want and idx.to_bytes() == bm.to_bytes(want)
    if row.facts:
        row.facts(got)
    t = la.last_bam_index_times(caller)
    assert (t["n_recs"], t["n_from_device"], t["first_bad_record"], t["n_launches"]) == (n_recs, 0, -1, 4 if n_recs else 0)
    assert t["n_chunks"] >= sum(len(cs) for r in got["refs"] for cs in r["bins"].values())       # (before bins and chunks merge)
    idx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_golden_from_host_memory(caller, kind):
    import lofreq_amd as la
    f = load(kind)
    idx = la.bam_index_build(caller, f.data, f.rec_off, f.data_off, f.comp_off, 0, len(f.refs))
    assert content(idx) == f.want
    assert la.last_bam_index_times(caller)["n_from_device"] == 0
    assert la.BamIndex.from_bytes(idx.to_bytes()).to_bytes() == idx.to_bytes() == bm.to_bytes(f.want)
    idx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_golden_from_the_resident_inflate_result(caller, kind):
    """lfq_bgzf_inflate of the file, then the index of the records where the result holds them: taken from the device copy, with
    the result's own block tables (the end-of-file marker is no block of the index's)"""
    import lofreq_amd as la
    from lofreq_amd import _lib
    L = _lib.load()
    f = load(kind)
    comp = np.frombuffer(f.bam, np.uint8).copy()
    res = C.POINTER(_lib.BgzfResult)()
    assert L.lfq_bgzf_inflate(caller.h, comp.ctypes.data, len(comp), C.byref(res)) == 0
    r = res.contents
    nb = int(r.n_blocks)
    data_off = np.ctypeslib.as_array(C.cast(r.data_off, C.POINTER(C.c_int64)), (nb + 1,)).tolist()
    comp_off = np.ctypeslib.as_array(C.cast(r.comp_off, C.POINTER(C.c_int64)), (nb + 1,)).tolist()
    while nb and data_off[nb] == data_off[nb - 1]:
        nb -= 1
    assert nb == len(f.data_off) - 1 and data_off[:nb + 1] == f.data_off and comp_off[:nb + 1] == f.comp_off
    idx = la.bam_index_build(caller, (r.data, int(r.n_bytes)), f.rec_off, data_off[:nb + 1], comp_off[:nb + 1], 0, len(f.refs))
    t = la.last_bam_index_times(caller)
    assert t["n_from_device"] == 1 and t["n_recs"] == len(f.rec_off) - 1 and t["n_launches"] == 4
    assert content(idx) == f.want
    # the inflate result is still the context's
    assert C.string_at(r.data, int(r.n_bytes)) == f.data
    idx.close()


def test_a_second_build_gives_identical_bytes(caller):
    import lofreq_amd as la
    f = load("python")
    a = la.bam_index_build(caller, f.data, f.rec_off, f.data_off, f.comp_off, 0, len(f.refs))
    small = _build(la, caller, ROWS["one_record"])
    b = la.bam_index_build(caller, f.data, f.rec_off, f.data_off, f.comp_off, 0, len(f.refs))
    assert a.to_bytes() == b.to_bytes() and small.to_bytes() != a.to_bytes()
    for i in (a, b, small):
        i.close()


# ---- the chain, and back --------------------------------------------------------------------------------------------------------------

def _fetch(la, caller, file_bytes, chunks, ref, **opts):
    """the records a query's chunks hold under the scan options: per chunk, the blocks it names go through
    lfq_readset_create_from_bgzf from the chunk's first byte to its last -> the file-wide offsets of the kept records"""
    data, data_off, comp_off = bm.file_tables(file_bytes)
    comp_off, data_off = comp_off + [len(file_bytes)], data_off + [len(data)]       # (the marker's place, for a chunk that ends there)
    block_of = {o: b for b, o in enumerate(comp_off)}
    kept = []
    for cb, ce in chunks:
        b0, b1 = block_of[cb >> 16], block_of[ce >> 16]
        last = b1 if ce & 0xffff else b1 - 1
        comp = np.frombuffer(file_bytes[comp_off[b0]:comp_off[last + 1]], np.uint8).copy()
        stop = data_off[b1] - data_off[b0] + (ce & 0xffff)
        rs = la.ReadSet.from_bgzf(caller, comp, cb & 0xffff, ref, stop=stop, **opts)
        assert rs.n == len(rs.kept["pos"])
        kept += [data_off[b0] + int(o) - 36 for o in rs.kept["data_off"][:rs.n]]
        rs.close()
    return data, kept


def _round_trip(la, caller, file_bytes, idx, ref, tid, regions):
    data = bm.file_tables(file_bytes)[0]
    rec_off = bm.record_chain(data, bm.parse_header(data)[0])
    n_found = 0
    for beg, end in regions:
        chunks = idx.query(tid, beg, end)
        _, kept = _fetch(la, caller, file_bytes, chunks, ref, tid=tid, beg=beg, end=end, flag_mask=4)
        want = [rec_off[j] for j in bm.overlapping(data, rec_off, tid, beg, end)]
        assert sorted(kept) == want and len(set(kept)) == len(kept), (tid, beg, end, len(kept), len(want))
        n_found += len(want)
    return n_found


def test_chain_encode_frame_cuts_deflate_index(caller, tmp_path):
    """the records of tests/golden/bam_write.json, sorted: encode -> frame -> bam_record_cuts -> lfq_bgzf_deflate and
    lfq_bam_index_build of framed->data by pointer, behind a header compressed by the same call"""
    import lofreq_amd as la
    import bam_write_model as wm
    from lofreq_amd import _lib
    from lofreq_amd.pileup import bgzf_deflated_arrays
    L = _lib.load()
    fx = json.load(open(GOLDEN))
    genome = fx["genome"].encode()
    recs = golden_records(sorted(fx["input"], key=lambda r: r[0]), genome)
    n = len(recs["pos"])
    rs = la.ReadSet.from_bam_records(caller, recs["data"], recs["data_off"], recs["pos"], recs["flag"], recs["mapq"], recs["l_qname"],
                                     recs["n_cigar"], recs["l_qseq"], recs["ref"])
    enc = rs.encode_bam(recs, None, wm.DROP_ALN_TAGS)
    head_blocks = la.bgzf_deflate(caller, bm.header([("chr1", len(genome))]))[0]
    cores = np.frombuffer(b"".join(struct.pack("<iiBBHHHiiii", 0, int(recs["pos"][i]), int(recs["l_qname"][i]), int(recs["mapq"][i]),
                                               0xdead, int(recs["n_cigar"][i]), int(recs["flag"][i]), int(recs["l_qseq"][i]), -1, -1, 0)
                                   for i in range(n)), np.uint8).copy()
    fr = C.POINTER(_lib.BamFramed)()
    assert L.lfq_bam_frame_encoded(caller.h, cores.ctypes.data, n, C.byref(fr)) == 0
    n_bytes = int(fr.contents.n_bytes)
    rec_off = np.ctypeslib.as_array(C.cast(fr.contents.rec_off, C.POINTER(C.c_int64)), (n + 1,)).copy()
    cuts = la.bam_record_cuts(rec_off, 700)
    assert len(cuts) >= 4 and set(cuts.tolist()) <= set(rec_off.tolist())
    out = C.POINTER(_lib.BgzfDeflated)()
    assert L.lfq_bgzf_deflate(caller.h, fr.contents.data, n_bytes, cuts.ctypes.data, len(cuts), _lib.LFQ_BGZF_PUT_EOF, C.byref(out)) == 0
    comp, comp_off, data_off, _ = bgzf_deflated_arrays(out.contents)
    body_before = C.string_at(fr.contents.data, n_bytes)
    idx = la.bam_index_build(caller, (fr.contents.data, n_bytes), rec_off, data_off, comp_off, len(head_blocks), 1)
    t = la.last_bam_index_times(caller)
    assert t["n_from_device"] == 1 and t["n_recs"] == n and t["first_bad_record"] == -1
    # the frame and deflate results are still the context's, untouched
    assert C.string_at(fr.contents.data, n_bytes) == body_before and int(fr.contents.n_reads) == n
    again = bgzf_deflated_arrays(out.contents)
    assert again[0].tobytes() == comp.tobytes() and again[1].tolist() == comp_off.tolist()
    # the file as written, and the model on its bytes
    file_bytes = head_blocks.tobytes() + comp.tobytes()
    assert file_bytes.endswith(bz.EOF_BLOCK)
    want, data = bm.build_from_file(file_bytes)[:2]
    got = content(idx)
    assert got == want and got["refs"][0]["meta"][1] == [int((recs["flag"] & 4 == 0).sum()), int((recs["flag"] & 4 != 0).sum())]
    assert data[bm.parse_header(data)[0]:] == body_before
    bai = idx.to_bytes()
    if os.path.exists(LOFREQ):                              # (only this comparison depends on the binary being at hand)
        path = str(tmp_path / "out.bam")
        open(path, "wb").write(file_bytes)
        open(path + ".bai", "wb").write(bai)                # the library's index: the binary reads the counts from it
        stats = subprocess.run([LOFREQ, "idxstats", path], check=True, capture_output=True, text=True).stdout.split("\n")
        assert stats[0].split("\t") == ["chr1", str(len(genome))] + [str(v) for v in got["refs"][0]["meta"][1]], stats
        os.remove(path + ".bai")
        subprocess.run([LOFREQ, "index", path], check=True, capture_output=True)
        assert bm.parse_bai(open(path + ".bai", "rb").read()) == got
    # and back: regions at the edges of records and of the one chunk there is
    spans = [bm.record_span(body_before, int(o)) for o in rec_off[:-1]]
    regions = [(0, len(genome)), (0, 1), (len(genome) - 1, len(genome))]
    for _, b, e, mapped in spans[:3] + spans[-3:]:
        regions += [(b, b + 1), (e - 1, e), (e, e + 1), (max(b - 1, 0), b)]
    assert _round_trip(la, caller, file_bytes, idx, genome, 0, regions) > n
    rs.close()
    idx.close()


def test_query_round_trip_on_the_golden(caller):
    """chrD of the fixture -- 150 reads over 18 windows in blocks of mixed sizes --: for regions at chunks' and windows' edges the
    blocks the chunks name hold exactly the brute-force records"""
    import lofreq_amd as la
    f = load("python")
    idx = la.bam_index_build(caller, f.data, f.rec_off, f.data_off, f.comp_off, 0, len(f.refs))
    assert len(idx.bins(3)) >= 10
    starts = {u: j for j, u in enumerate(f.us)}
    regions = [(0, 300000), (5 << 14, 6 << 14), ((5 << 14) - 1, 5 << 14), (5 << 14, (5 << 14) + 1)]
    for b in sorted(idx.bins(3))[:3] + sorted(idx.bins(3))[-2:]:
        for cb, _ in idx.bins(3)[b][:1]:
            _, beg, end, _ = f.spans[starts[cb]]            # the record a chunk begins with
            regions += [(beg, beg + 1), (end - 1, end), (end, end + 1), (max(beg - 1, 0), beg)]
    n_found = _round_trip(la, caller, f.bam, idx, b"A" * 300000, 3, regions)
    assert n_found >= 150 + len(regions) // 4
    idx.close()
