"""VCF text parsed on the device and `lofreq vcfset` (include/lofreq_amd.h: lfq_vcf_*, lfq_vcfset).

    v = Vcf.open(caller, data)                      # bytes / uint8 array of an UNCOMPRESSED VCF; a view from bgzf_inflate_view stays on the device
    v.records(), v.header(), v.filter_vars()        # the record table, the header text, lfq_filter_var structs for filter_vars
    v.uniq_variants("chr1"), v.ign_mask("chr1", n)  # what ReadSet.uniq and ReadSet.source_qual(ign=...) take
    dbsnp = Vcf.open(caller, data2, tabix=True)     # the second file of vcfset
    out = vcfset(v, dbsnp, op="complement")         # {"text", "keep", "n_vars1", "n_ignored", "n_out"}
    gz, tbi = vcf_write_gz(caller, out["text"])     # the .vcf.gz and its .tbi as they go to disk
    idx = VcfIndex.from_file_bytes(caller, tbi)     # or dbsnp.index(data_off, comp_off) of a file just inflated or deflated
    part = Vcf.open_indexed(caller, gz, idx, "chr1", 1000, 2000)       # only the blocks the region needs are inflated
"""
import ctypes as C
import struct

import numpy as np

from . import _lib

VCF_LINE_TOO_LONG, VCF_NUL, VCF_NUMBER, VCF_FIELDS, VCF_UNSORTED, VCF_INTERVAL, VCF_MULTIALLELIC, VCF_RANGE = 1, 2, 3, 4, 5, 6, 7, 8
VCF_F_PASSES, VCF_F_FILTERED, VCF_F_INDEL_LEN, VCF_F_INDEL_KEY, VCF_F_ALT_COMMA = 1, 2, 4, 8, 16
VCFSET_OPS = {"intersect": 0, "complement": 1, "concat": 2}
VCFSET_DROPPED, VCFSET_IGNORED, VCFSET_TAKEN, VCFSET_WRITTEN = 0, 1, 2, 3


class VcfError(ValueError):
    """a VCF or a vcfset call is refused: .why (VCF_*), .file (0: the first file, 1: the second, 2 + i: a further file of concat),
    .line (1-based)"""

    def __init__(self, why, file, line):
        ValueError.__init__(self, "VCF refused: %s at line %d of file %d" % (
            {1: "line too long", 2: "NUL byte", 3: "number too long", 4: "fewer than five fields", 5: "not sorted",
             6: "no interval", 7: "multi-allelic", 8: "interval beyond what a .tbi holds"}.get(why, why), line, file))
        self.why, self.file, self.line = why, file, line


def _name(name):
    return name.encode("latin-1") if isinstance(name, str) else bytes(name)


def _arr(ptr, n, dtype):
    if not n or not ptr:
        return np.zeros(0, dtype)
    return np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr), dtype).copy()


class Vcf:
    """lfq_vcf: the file's bytes resident and parsed"""

    def __init__(self, caller, h, keep):
        self.caller, self.h, self._keep = caller, h, keep
        if not hasattr(caller, "_vcfs"):
            import weakref
            caller._vcfs = weakref.WeakSet()
        caller._vcfs.add(self)                      # closed with the caller, in front of its context (SnvCaller.close)

    @staticmethod
    def open(caller, data, tabix=False, file=0):
        a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8)
        h, why, line = C.c_void_p(), C.c_int(0), C.c_int64(0)
        rc = _lib.load().lfq_vcf_open(caller.h, a.ctypes.data if len(a) else None, len(a), 1 if tabix else 0, C.byref(h), C.byref(why),
                                      C.byref(line))
        if rc == -1 and why.value != 0:             # LFQ_ERR_INVALID with a reason: the file, not the call
            raise VcfError(int(why.value), file, int(line.value))
        _lib.check(rc, "lfq_vcf_open")
        return Vcf(caller, h, a)

    @staticmethod
    def open_indexed(caller, comp, index, chrom, beg, end, file=1):
        """lfq_vcf_open_indexed: the records of `chrom` overlapping [beg, end) -- and possibly more, never less -- of the whole .vcf.gz
        `comp`, through its VcfIndex: only the blocks the region's chunks lie in are inflated.  Replaces the caller's live inflate
        result"""
        a = np.frombuffer(comp, np.uint8) if isinstance(comp, (bytes, bytearray, memoryview)) else np.ascontiguousarray(comp, np.uint8)
        h, why, line = C.c_void_p(), C.c_int(0), C.c_int64(0)
        rc = _lib.load().lfq_vcf_open_indexed(caller.h, a.ctypes.data if len(a) else None, len(a), index.h, _name(chrom), int(beg), int(end),
                                              C.byref(h), C.byref(why), C.byref(line))
        if rc == -1 and why.value != 0:
            raise VcfError(int(why.value), file, int(line.value))
        _lib.check(rc, "lfq_vcf_open_indexed")
        return Vcf(caller, h, a)

    def index(self, data_off, comp_off, file_off=0, file=0):
        """lfq_vcf_index_build -> VcfIndex of this file (opened with tabix=True), whose text lies in the BGZF blocks data_off / comp_off
        [n_blocks + 1] describe, as bgzf_deflate and bgzf_inflate_view give them.  VcfError(VCF_RANGE) with the first line a .tbi
        cannot hold"""
        do, co = np.ascontiguousarray(data_off, np.int64), np.ascontiguousarray(comp_off, np.int64)
        if len(do) < 1 or len(do) != len(co):
            raise ValueError("Vcf.index: data_off and comp_off take n_blocks + 1 entries each")
        out, why, line = C.c_void_p(), C.c_int(0), C.c_int64(0)
        rc = _lib.load().lfq_vcf_index_build(self.h, do.ctypes.data, co.ctypes.data, len(do) - 1, int(file_off), C.byref(out), C.byref(why),
                                             C.byref(line))
        if rc == -1 and why.value != 0:
            raise VcfError(int(why.value), file, int(line.value))
        _lib.check(rc, "lfq_vcf_index_build")
        return VcfIndex(out)

    @property
    def n_records(self):
        return int(_lib.load().lfq_vcf_n_records(self.h))

    @property
    def n_lines_behind(self):
        return int(_lib.load().lfq_vcf_n_lines_behind(self.h))

    def header(self):
        """-> (text: bytes, found: bool)"""
        p, n, found = C.c_void_p(), C.c_int64(0), C.c_int(0)
        _lib.check(_lib.load().lfq_vcf_header(self.h, C.byref(p), C.byref(n), C.byref(found)), "lfq_vcf_header")
        return (C.string_at(p, int(n.value)) if n.value else b""), bool(found.value)

    def records(self):
        """lfq_vcf_records -> dict of arrays per record (line, pos, qual, flags, n_fields, field_off[n, 10], run_id) and line_start,
        run_begin, run_name"""
        t = _lib.VcfTable()
        _lib.check(_lib.load().lfq_vcf_records(self.h, C.byref(t)), "lfq_vcf_records")
        n, nl, nr = int(t.n_records), int(t.n_lines), int(t.n_runs)
        return {"line": _arr(t.line, n, np.int64), "pos": _arr(t.pos, n, np.int64), "qual": _arr(t.qual, n, np.int32),
                "flags": _arr(t.flags, n, np.uint8), "n_fields": _arr(t.n_fields, n, np.uint8),
                "field_off": _arr(t.field_off, n * 10, np.uint16).reshape(n, 10), "run_id": _arr(t.run_id, n, np.int32),
                "line_start": _arr(t.line_start, nl + 1 if nl else 0, np.int64), "run_begin": _arr(t.run_begin, nr + 1, np.int64),
                "run_name": [t.run_name[i] for i in range(nr)]}

    def filter_vars(self):
        """lfq_vcf_filter_vars -> FILTER_VAR_DTYPE array, ready for caller.filter_vars / lfq_filter_vars"""
        out = np.zeros(self.n_records, _lib.FILTER_VAR_DTYPE)
        _lib.check(_lib.load().lfq_vcf_filter_vars(self.h, out.ctypes.data if len(out) else None), "lfq_vcf_filter_vars")
        return out

    def uniq_variants(self, chrom, only_unfiltered=True, uni_freq=0.0):
        """lfq_vcf_uniq_variants -> {"pos", "ref": [bytes], "alt": [bytes], "indel_key", "af", "line"}: what ReadSet.uniq takes"""
        v, lines, bad = _lib.UniqVariants(), C.c_void_p(), C.c_int64(0)
        rc = _lib.load().lfq_vcf_uniq_variants(self.h, _name(chrom), 1 if only_unfiltered else 0, float(uni_freq), C.byref(v), C.byref(lines),
                                               C.byref(bad))
        if rc == -1 and bad.value > 0:
            raise VcfError(0, 0, int(bad.value))
        _lib.check(rc, "lfq_vcf_uniq_variants")
        n = int(v.n)
        ro, ao = _arr(v.ref_off, n + 1, np.int64), _arr(v.alt_off, n + 1, np.int64)
        ref = C.string_at(v.ref, int(ro[-1])) if n else b""
        alt = C.string_at(v.alt, int(ao[-1])) if n else b""
        return {"pos": _arr(v.pos, n, np.int64), "ref": [ref[ro[i]:ro[i + 1]] for i in range(n)], "alt": [alt[ao[i]:ao[i + 1]] for i in range(n)],
                "indel_key": _arr(v.indel_key_or_null, n, np.uint8), "af": _arr(v.af, n, np.float32), "line": _arr(lines.value, n, np.int64)}

    def ign_mask(self, chrom, ref_len, bed=None, mask=None):
        """lfq_vcf_ign_mask: ORs the positions of `chrom` into mask (a new one of ref_len bytes when None) and returns it"""
        if mask is None:
            mask = np.zeros(int(ref_len), np.uint8)
        assert mask.dtype == np.uint8 and mask.flags.c_contiguous and len(mask) >= ref_len
        _lib.check(_lib.load().lfq_vcf_ign_mask(self.h, _name(chrom), int(ref_len), bed.h if bed is not None else None,
                                                mask.ctypes.data if len(mask) else None), "lfq_vcf_ign_mask")
        return mask

    def close(self):
        if getattr(self, "h", None):
            _lib.load().lfq_vcf_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def vcfset(one, two=None, more=(), op="intersect", only_passed=False, only_pos=False, only_snvs=False, only_indels=False,
           count_only=False, add_info=None):
    """lfq_vcfset -> {"text": bytes, "keep": uint8 array (VCFSET_*), "n_vars1", "n_ignored", "n_out"}; VcfError where the reference
    stops (a multi-allelic record of the first file)"""
    conf = _lib.VcfsetConf(VCFSET_OPS[op] if isinstance(op, str) else int(op), int(only_passed), int(only_pos), int(only_snvs),
                           int(only_indels), int(count_only), _name(add_info) if add_info else None)
    arr = (C.c_void_p * max(len(more), 1))(*[m.h for m in more])
    out = C.POINTER(_lib.VcfsetResult)()
    rc = _lib.load().lfq_vcfset(one.h, two.h if two is not None else None, arr, len(more), C.byref(conf), C.byref(out))
    if rc == -1 and out and out.contents.why != 0:
        r = out.contents
        raise VcfError(int(r.why), int(r.bad_file) + (1 if r.bad_file > 0 else 0), int(r.bad_line))
    _lib.check(rc, "lfq_vcfset")
    r = out.contents
    return {"text": C.string_at(r.text, int(r.text_bytes)) if r.text_bytes else b"", "keep": _arr(r.keep, int(r.n_keep), np.uint8),
            "n_vars1": int(r.n_vars1), "n_ignored": int(r.n_ignored), "n_out": int(r.n_out)}


def last_vcf_times(caller):
    """lfq_last_vcf_times -> dict of the struct's fields"""
    t = _lib.VcfTimes()
    _lib.check(_lib.load().lfq_last_vcf_times(caller.h, C.byref(t)), "lfq_last_vcf_times")
    return {k: getattr(t, k) for k, _ in _lib.VcfTimes._fields_ if k != "pad_"}


META_BIN = 37450


class VcfIndex:
    """an lfq_vcf_index (a host object, freed with this one): the tabix index of a bgzipped VCF.  names -> [bytes] in the file's
    order; bins(name) -> {bin: [(chunk begin, chunk end)]} without the metadata pseudo-bin, linear(name) -> the 16 KiB windows'
    offsets, meta(name) -> None or ((u of the first record, v of the last), (records, 0)), n_no_coor, query(name, beg, end) ->
    [(begin, end)] virtual offsets; to_bytes() the uncompressed .tbi, to_file_bytes(caller) the file as it goes to disk"""

    def __init__(self, handle):
        self.h = handle
        self._parsed = None

    @classmethod
    def from_bytes(cls, tbi):
        a = np.frombuffer(bytes(tbi), np.uint8)
        out = C.c_void_p()
        _lib.check(_lib.load().lfq_vcf_index_parse(a.ctypes.data if len(a) else None, len(a), C.byref(out)), "lfq_vcf_index_parse")
        return cls(out)

    @classmethod
    def from_file_bytes(cls, caller, tbi_file):
        """a .tbi as it lies on disk: BGZF, inflated with bgzf_inflate (which replaces the caller's live inflate result)"""
        from .pileup import bgzf_inflate
        return cls.from_bytes(bgzf_inflate(caller, tbi_file)[0].tobytes())

    def close(self):
        if self.h:
            _lib.load().lfq_vcf_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def to_bytes(self):
        p, n = C.c_void_p(), C.c_int64()
        _lib.check(_lib.load().lfq_vcf_index_bytes(self.h, C.byref(p), C.byref(n)), "lfq_vcf_index_bytes")
        return C.string_at(p, n.value)

    def to_file_bytes(self, caller):
        """the .tbi as it goes to disk: BGZF-compressed with bgzf_deflate, the end-of-file block behind it"""
        from .pileup import bgzf_deflate
        return bgzf_deflate(caller, self.to_bytes(), eof=True)[0].tobytes()

    @property
    def names(self):
        L = _lib.load()
        return [L.lfq_vcf_index_name(self.h, i) for i in range(int(L.lfq_vcf_index_n_names(self.h)))]

    def _refs(self):
        if self._parsed is None:
            tbi = self.to_bytes()
            n_ref, l_nm = struct.unpack_from("<i", tbi, 4)[0], struct.unpack_from("<i", tbi, 32)[0]
            o, refs = 36 + l_nm, []
            for _ in range(n_ref):
                n_bin, = struct.unpack_from("<i", tbi, o)
                o += 4
                bins, meta = {}, None
                for _ in range(n_bin):
                    b, n_chunk = struct.unpack_from("<Ii", tbi, o)
                    v = struct.unpack_from("<%dQ" % (2 * n_chunk), tbi, o + 8)
                    o += 8 + 16 * n_chunk
                    chunks = [(v[2 * k], v[2 * k + 1]) for k in range(n_chunk)]
                    if b == META_BIN:
                        meta = tuple(chunks)
                    else:
                        bins[b] = chunks
                n_intv, = struct.unpack_from("<i", tbi, o)
                refs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, tbi, o + 4)), meta))
                o += 4 + 8 * n_intv
            self._parsed = (refs, struct.unpack_from("<Q", tbi, o)[0], list(struct.unpack_from("<6i", tbi, 8)))
        return self._parsed

    def _ref(self, name):
        return self._refs()[0][self.names.index(_name(name))]

    @property
    def n_no_coor(self):
        return self._refs()[1]

    @property
    def conf(self):
        """[format, col_seq, col_beg, col_end, meta, skip]"""
        return self._refs()[2]

    def bins(self, name):
        return self._ref(name)[0]

    def linear(self, name):
        return self._ref(name)[1]

    def meta(self, name):
        return self._ref(name)[2]

    def query(self, name, beg, end):
        b, e, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        _lib.check(_lib.load().lfq_vcf_index_query(self.h, _name(name), int(beg), int(end), C.byref(b), C.byref(e), C.byref(n)),
                   "lfq_vcf_index_query")
        if not n.value:
            return []
        get = lambda p: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), (n.value,)).tolist()
        return list(zip(get(b), get(e)))


def last_vcf_index_times(caller):
    """lfq_last_vcf_index_times -> dict(kernels_ms, download_ms, host_ms, n_records, n_chunks, n_intervals, n_launches)"""
    t = _lib.VcfIndexTimes()
    _lib.check(_lib.load().lfq_last_vcf_index_times(caller.h, C.byref(t)), "lfq_last_vcf_index_times")
    return {k: getattr(t, k) for k, _ in _lib.VcfIndexTimes._fields_ if k != "pad_"}


def vcf_write_gz(caller, text):
    """VCF text -> (the .vcf.gz, its .tbi), both as they go to disk: a tabix-mode open, cuts that keep lines whole (bam_record_cuts over
    the line starts, as the binary's blocks end on line boundaries), bgzf_deflate with the end-of-file block, the index over the
    deflate result's own tables, and the index compressed.  VcfError where the text cannot be indexed"""
    from .bamindex import bam_record_cuts
    from .pileup import bgzf_deflate
    a = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, np.uint8)
    v = Vcf.open(caller, a, tabix=True)
    try:
        starts = v.records()["line_start"]
        cuts = bam_record_cuts(np.append(starts[:-1], len(a))) if len(starts) > 1 else None
        comp, comp_off, data_off, _ = bgzf_deflate(caller, a, cuts=cuts, eof=True)
        idx = v.index(data_off, comp_off)
    finally:
        v.close()
    return comp.tobytes(), idx.to_file_bytes(caller)
