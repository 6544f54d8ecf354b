"""The index of a BAM (include/lofreq_amd.h: lfq_bam_index_*): its .bai built on the device from the records and the BGZF block
tables of a file being written or read, serialised, parsed and queried; and the two host loops of a writer, lfq_bam_record_chain
and lfq_bam_record_cuts."""
import ctypes as C
import struct

import numpy as np

from . import _lib

META_BIN = 37450


class BamIndexError(RuntimeError):
    """lfq_bam_index_build refused its input; .record: the first bad record, -1 when an argument was refused"""

    def __init__(self, msg, record):
        RuntimeError.__init__(self, msg)
        self.record = record


def _i64(a):
    return np.ascontiguousarray(a, np.int64)


class BamIndex:
    """an lfq_bam_index (a host object, freed with this one).  bins(tid) -> {bin: [(chunk begin, chunk end)]} without the metadata
    pseudo-bin, linear(tid) -> the 16 KiB windows' offsets, meta(tid) -> None or ((u of the first record, v of the last), (mapped,
    unmapped)), n_no_coor, query(tid, beg, end) -> [(begin, end)] virtual offsets, to_bytes() -> the .bai"""

    def __init__(self, handle):
        self.h = handle
        self._parsed = None

    @classmethod
    def from_bytes(cls, bai):
        a = np.frombuffer(bytes(bai), np.uint8)
        out = C.c_void_p()
        _lib.check(_lib.load().lfq_bam_index_parse(a.ctypes.data if len(a) else None, len(a), C.byref(out)), "lfq_bam_index_parse")
        return cls(out)

    def close(self):
        if self.h:
            _lib.load().lfq_bam_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def to_bytes(self):
        p, n = C.c_void_p(), C.c_int64()
        _lib.check(_lib.load().lfq_bam_index_bytes(self.h, C.byref(p), C.byref(n)), "lfq_bam_index_bytes")
        return C.string_at(p, n.value)

    def _refs(self):
        if self._parsed is None:
            bai = self.to_bytes()
            n_ref, = struct.unpack_from("<i", bai, 4)
            o, refs = 8, []
            for _ in range(n_ref):
                n_bin, = struct.unpack_from("<i", bai, o)
                o += 4
                bins, meta = {}, None
                for _ in range(n_bin):
                    b, n_chunk = struct.unpack_from("<Ii", bai, o)
                    v = struct.unpack_from("<%dQ" % (2 * n_chunk), bai, o + 8)
                    o += 8 + 16 * n_chunk
                    chunks = [(v[2 * k], v[2 * k + 1]) for k in range(n_chunk)]
                    if b == META_BIN:
                        meta = tuple(chunks)
                    else:
                        bins[b] = chunks
                n_intv, = struct.unpack_from("<i", bai, o)
                refs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, bai, o + 4)), meta))
                o += 4 + 8 * n_intv
            self._parsed = (refs, struct.unpack_from("<Q", bai, o)[0])
        return self._parsed

    @property
    def n_ref(self):
        return len(self._refs()[0])

    @property
    def n_no_coor(self):
        return self._refs()[1]

    def bins(self, tid):
        return self._refs()[0][tid][0]

    def linear(self, tid):
        return self._refs()[0][tid][1]

    def meta(self, tid):
        return self._refs()[0][tid][2]

    def query(self, tid, beg, end):
        b, e, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        _lib.check(_lib.load().lfq_bam_index_query(self.h, int(tid), int(beg), int(end), C.byref(b), C.byref(e), C.byref(n)),
                   "lfq_bam_index_query")
        if not n.value:
            return []
        get = lambda p: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), (n.value,)).tolist()
        return list(zip(get(b), get(e)))


def bam_index_build(caller, body, rec_off, data_off, comp_off, file_off, n_ref):
    """lfq_bam_index_build -> BamIndex.  body: bytes or a uint8 array, or (address, n_bytes) of memory that lives elsewhere -- such
    as the `data` of the caller's live lfq_bam_framed or lfq_bgzf_result, which is then read from its device copy.  rec_off
    [n_recs + 1], data_off and comp_off [n_blocks + 1].  Raises BamIndexError with the first bad record."""
    L = _lib.load()
    if isinstance(body, tuple):
        addr, n_bytes = int(body[0]), int(body[1])
    else:
        a = np.ascontiguousarray(np.frombuffer(body, np.uint8) if isinstance(body, (bytes, bytearray, memoryview)) else body, np.uint8)
        addr, n_bytes = (a.ctypes.data if len(a) else None), len(a)
    ro, do, co = _i64(rec_off), _i64(data_off), _i64(comp_off)
    if len(ro) < 1 or len(do) < 1 or len(do) != len(co):
        raise BamIndexError("bam_index_build: rec_off takes n_recs + 1 entries, data_off and comp_off n_blocks + 1 each", -1)
    out = C.c_void_p()
    rc = L.lfq_bam_index_build(caller.h, addr, n_bytes, ro.ctypes.data, len(ro) - 1, do.ctypes.data, co.ctypes.data, len(do) - 1,
                               int(file_off), int(n_ref), C.byref(out))
    if rc != _lib.LFQ_OK:
        bad = last_bam_index_times(caller)["first_bad_record"] if rc == -1 else -1
        raise BamIndexError("lfq_bam_index_build failed: %s (%d)%s" % (L.lfq_strerror(rc).decode(), rc,
                                                                      ", record %d" % bad if bad >= 0 else ""), bad)
    return BamIndex(out)


def last_bam_index_times(caller):
    """lfq_last_bam_index_times -> dict(upload_ms, kernels_ms, download_ms, host_ms, n_recs, n_chunks, n_intervals,
    first_bad_record, n_launches, n_from_device)"""
    t = _lib.BamIndexTimes()
    _lib.check(_lib.load().lfq_last_bam_index_times(caller.h, C.byref(t)), "lfq_last_bam_index_times")
    return {k: getattr(t, k) for k, _ in _lib.BamIndexTimes._fields_}


def bam_record_chain(bam, first=0, stop=None):
    """lfq_bam_record_chain (host only): rec_off [n + 1] of every complete record of bam[first:stop]"""
    L = _lib.load()
    a = np.ascontiguousarray(np.frombuffer(bam, np.uint8) if isinstance(bam, (bytes, bytearray, memoryview)) else bam, np.uint8)
    p, n = C.POINTER(C.c_int64)(), C.c_int64()
    keep = a if len(a) else np.zeros(1, np.uint8)
    _lib.check(L.lfq_bam_record_chain(keep.ctypes.data, int(first), len(a) if stop is None else int(stop), C.byref(p), C.byref(n)),
               "lfq_bam_record_chain")
    try:
        return np.ctypeslib.as_array(p, (n.value + 1,)).copy()
    finally:
        L.lfq_bam_record_chain_free(p)


def bam_record_cuts(rec_off, max_piece=65280):
    """lfq_bam_record_cuts (host only): the cuts for bgzf_deflate that keep records whole where they fit"""
    L = _lib.load()
    ro = _i64(rec_off)
    p, n = C.POINTER(C.c_int64)(), C.c_int64()
    _lib.check(L.lfq_bam_record_cuts(ro.ctypes.data, len(ro) - 1, int(max_piece), C.byref(p), C.byref(n)), "lfq_bam_record_cuts")
    try:
        return np.ctypeslib.as_array(p, (n.value,)).copy() if n.value else np.zeros(0, np.int64)
    finally:
        L.lfq_bam_record_cuts_free(p)
