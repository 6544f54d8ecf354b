"""`lofreq faidx`, the contig in front of every region and `lofreq checkref` (include/lofreq_amd.h: lfq_fasta_*, lfq_checkref,
lfq_bgzf_gzi_bytes): the file resident on the device, its index built there, whole contigs fetched there.

    fa = Fasta.open(caller, data)               # bytes / uint8 array; a view from bgzf_inflate_view stays on the device
    idx = FastaIndex.build(fa)                  # FastaError where `lofreq faidx` refuses the file
    open("x.fa.fai", "w").write(idx.to_text())
    ref = fa.fetch(idx, "chr1")                 # Contig: bytes(ref), ref.seq_ptr; ReadSet.from_arrays(..., ref=ref) takes it on the device
"""
import ctypes as C

import numpy as np

from . import _lib

FASTA_UNEXPECTED, FASTA_LINE_LENGTH, FASTA_LAST_EMPTY, FASTA_EMPTY_FILE = 1, 2, 3, 4
PATH_NONE, PATH_REGULAR, PATH_GENERAL = 0, 1, 2
CHECKREF_OK, CHECKREF_NO_SEQUENCE, CHECKREF_LENGTH = 0, 1, 2


class FastaError(ValueError):
    """lfq_fasta_index_build refused the file: .why (FASTA_*), .line (1-based, 0: the file as a whole), .byte (the offending line's
    first byte, or the one behind a leading '\\r'; -1: the file ends there)"""

    def __init__(self, why, line, byte):
        ValueError.__init__(self, "FASTA refused: %s at line %d" % ({1: "unexpected byte", 2: "different line length",
                                                                    3: "the last entry has no sequence", 4: "no sequence"}.get(why, why), line))
        self.why, self.line, self.byte = why, line, byte


class FastaIndex:
    """lfq_fasta_index: build(fa) on the device, from_text(fai) from a .fai; to_text(), entries, n_duplicates"""

    def __init__(self, h):
        self.h = h

    @staticmethod
    def build(fa):
        L = _lib.load()
        h, why, line, byte = C.c_void_p(), C.c_int(0), C.c_int64(0), C.c_int(0)
        rc = L.lfq_fasta_index_build(fa.h, C.byref(h), C.byref(why), C.byref(line), C.byref(byte))
        if rc == -1 and why.value != 0:             # LFQ_ERR_INVALID with a reason: the file, not the call
            raise FastaError(int(why.value), int(line.value), int(byte.value))
        _lib.check(rc, "lfq_fasta_index_build")
        return FastaIndex(h)

    @staticmethod
    def from_text(text):
        if isinstance(text, str):
            text = text.encode("latin-1")
        h = C.c_void_p()
        _lib.check(_lib.load().lfq_fasta_index_parse(text, len(text), C.byref(h)), "lfq_fasta_index_parse")
        return FastaIndex(h)

    def to_text(self):
        p, n = C.c_void_p(), C.c_int64(0)
        _lib.check(_lib.load().lfq_fasta_index_text(self.h, C.byref(p), C.byref(n)), "lfq_fasta_index_text")
        return C.string_at(p, int(n.value)) if n.value else b""

    @property
    def entries(self):
        """[(name: bytes, length, offset, line_blen, line_len), ...] in file order"""
        L = _lib.load()
        out = []
        for i in range(L.lfq_fasta_index_n(self.h)):
            e = _lib.FastaEntry()
            _lib.check(L.lfq_fasta_index_entry(self.h, i, C.byref(e)), "lfq_fasta_index_entry")
            out.append((L.lfq_fasta_index_name(self.h, i), int(e.length), int(e.offset), int(e.line_blen), int(e.line_len)))
        return out

    @property
    def n_duplicates(self):
        return int(_lib.load().lfq_fasta_index_n_duplicates(self.h))

    def find(self, name):
        return int(_lib.load().lfq_fasta_index_find(self.h, _name(name)))

    def close(self):
        if getattr(self, "h", None):
            _lib.load().lfq_fasta_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _name(name):
    return name.encode("latin-1") if isinstance(name, str) else bytes(name)


class Contig:
    """what Fasta.fetch hands out: seq_ptr / d_seq_ptr (pinned host and device address of the same bytes), len; bytes(contig) copies.
    Valid until the next fetch on its Fasta or that file's close."""

    def __init__(self, fa, c):
        self.fa, self.seq_ptr, self.d_seq_ptr, self.len = fa, int(c.seq or 0), int(c.d_seq or 0), int(c.len)

    def __bytes__(self):
        return C.string_at(self.seq_ptr, self.len) if self.len else b""

    def __len__(self):
        return self.len


class Fasta:
    """lfq_fasta: the file's bytes resident and scanned"""

    def __init__(self, caller, h, keep):
        self.caller, self.h, self._keep = caller, h, keep
        if not hasattr(caller, "_fastas"):
            import weakref
            caller._fastas = weakref.WeakSet()
        caller._fastas.add(self)

    @staticmethod
    def open(caller, data):
        a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8)
        h = C.c_void_p()
        _lib.check(_lib.load().lfq_fasta_open(caller.h, a.ctypes.data if len(a) else None, len(a), C.byref(h)), "lfq_fasta_open")
        return Fasta(caller, h, a)

    def fetch(self, idx, name):
        out = C.POINTER(_lib.FastaContig)()
        _lib.check(_lib.load().lfq_fasta_fetch(self.h, idx.h, _name(name), C.byref(out)), "lfq_fasta_fetch")
        return Contig(self, out.contents)

    def close(self):
        if getattr(self, "h", None):
            _lib.load().lfq_fasta_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def last_fasta_times(caller):
    """lfq_last_fasta_times -> dict of the struct's fields"""
    t = _lib.FastaTimes()
    _lib.check(_lib.load().lfq_last_fasta_times(caller.h, C.byref(t)), "lfq_last_fasta_times")
    return {k: getattr(t, k) for k, _ in _lib.FastaTimes._fields_}


def checkref(idx, names, lens):
    """lfq_checkref: the @SQ names and lengths of a BAM header against the index -> (first_bad, why): (-1, CHECKREF_OK) when all
    match, else the first entry that does not and CHECKREF_NO_SEQUENCE / CHECKREF_LENGTH"""
    n = len(names)
    arr = (C.c_char_p * max(n, 1))(*[_name(x) for x in names])
    ln = np.ascontiguousarray(lens, np.int64)
    bad, why = C.c_int64(-1), C.c_int(0)
    _lib.check(_lib.load().lfq_checkref(idx.h, arr, ln.ctypes.data if n else None, n, C.byref(bad), C.byref(why)), "lfq_checkref")
    return int(bad.value), int(why.value)


class BgzfView:
    """the context's live lfq_bgzf_inflate result WITHOUT copies: .data is a view of the library's pinned bytes (valid until the
    caller's next inflate), which Fasta.open takes device to device"""

    def __init__(self, res):
        r = res.contents
        nb = int(r.n_blocks)
        self._res = res
        self.n_blocks = nb
        self.comp_off = np.ctypeslib.as_array(C.cast(r.comp_off, C.POINTER(C.c_int64)), (nb + 1,)).copy()
        self.data_off = np.ctypeslib.as_array(C.cast(r.data_off, C.POINTER(C.c_int64)), (nb + 1,)).copy()
        self.data = (np.ctypeslib.as_array(C.cast(r.data, C.POINTER(C.c_uint8)), (int(r.n_bytes),)) if r.n_bytes
                     else np.zeros(0, np.uint8))


def bgzf_inflate_view(caller, comp):
    a = np.frombuffer(comp, np.uint8) if isinstance(comp, (bytes, bytearray, memoryview)) else np.ascontiguousarray(comp, np.uint8)
    out = C.POINTER(_lib.BgzfResult)()
    _lib.check(_lib.load().lfq_bgzf_inflate(caller.h, a.ctypes.data if len(a) else None, len(a), C.byref(out)), "lfq_bgzf_inflate")
    return BgzfView(out)


def bgzf_gzi(view):
    """lfq_bgzf_gzi_bytes: the .gzi `lofreq faidx` writes beside a bgzip-compressed FASTA, from a BgzfView's block tables"""
    L = _lib.load()
    n = C.c_int64(0)
    _lib.check(L.lfq_bgzf_gzi_bytes(view._res, None, 0, C.byref(n)), "lfq_bgzf_gzi_bytes")
    buf = np.zeros(int(n.value), np.uint8)
    _lib.check(L.lfq_bgzf_gzi_bytes(view._res, buf.ctypes.data, len(buf), C.byref(n)), "lfq_bgzf_gzi_bytes")
    return buf.tobytes()
