"""Device-side pileup: reads of a region -> packed SNV tracks in HBM (`lfq_pileup_snv_tracks`),
what `compile_plp_col` (plp.c:797-1017) builds per column on the CPU."""
import ctypes as C

import numpy as np

from . import _lib
from .baq import _OPS

LFQ_NO_MAX_DEPTH = -1


class _MaxDepth:
    """lfq_set_max_depth on the caller's context for the duration of one call (None: no cap), back to none afterwards"""

    def __init__(self, caller, max_depth):
        self.h = caller.h
        self.v = LFQ_NO_MAX_DEPTH if max_depth is None else int(max_depth)

    def __enter__(self):
        _lib.check(_lib.load().lfq_set_max_depth(self.h, self.v), "lfq_set_max_depth")

    def __exit__(self, *exc):
        _lib.load().lfq_set_max_depth(self.h, LFQ_NO_MAX_DEPTH)


class DeviceTracks:
    """Tracks owned by the caller's context (valid until its next pileup call); quacks like a device PileupBatch."""

    on_device = True

    def __init__(self, tracks, col_pos):
        self._t = tracks
        self.ncols = int(tracks.ncols)
        self.max_col_obs = int(tracks.max_col_obs)
        self.col_pos = col_pos

    def _tracks(self):
        return self._t


def pileup_snv_tracks(caller, reads, ref, begin, end, lb=None, min_plp_bq=3, sq=None, max_depth=None):
    """reads: list of dicts {pos0, cigar [(op, len)], seq (codes 0..4), qual (phred), mapq, reverse};
    lb: list of the reads' lb tag bytes (from baq_batch) or None; sq: the reads' source-quality bytes (second
    result of source_qual_batch) or None; max_depth: -d of `lofreq call` (lfq_set_max_depth), None = no cap.
    -> DeviceTracks"""
    n = len(reads)
    pos = np.asarray([r["pos0"] for r in reads], np.int32)
    cig_off = np.zeros(n + 1, np.int64)
    seq_off = np.zeros(n + 1, np.int64)
    cig, seqs, quals = [], [], []
    for i, r in enumerate(reads):
        cig.extend((l << 4) | _OPS.index(o) for o, l in r["cigar"])
        cig_off[i + 1] = len(cig)
        seqs.append(np.asarray(r["seq"], np.uint8))
        quals.append(np.asarray(r["qual"], np.uint8))
        seq_off[i + 1] = seq_off[i] + len(seqs[-1])
    cig = np.asarray(cig if cig else [0], np.uint32)
    seq = np.concatenate(seqs) if seqs else np.zeros(1, np.uint8)
    qual = np.concatenate(quals) if quals else np.zeros(1, np.uint8)
    baq = None if lb is None else np.concatenate([np.asarray(x, np.uint8) for x in lb])
    mapq = np.asarray([r["mapq"] for r in reads] or [0], np.uint8)
    rev = np.asarray([1 if r["reverse"] else 0 for r in reads] or [0], np.uint8)
    ref = bytes(ref)
    rd = _lib.PileupReads()
    rd.n_reads = n
    rd.pos = pos.ctypes.data
    rd.cigar_off = cig_off.ctypes.data
    rd.cigar = cig.ctypes.data
    rd.seq_off = seq_off.ctypes.data
    rd.seq = seq.ctypes.data
    rd.qual = qual.ctypes.data
    rd.baq = baq.ctypes.data if baq is not None else None
    rd.mapq = mapq.ctypes.data
    rd.reverse = rev.ctypes.data
    rd.ref = C.cast(C.c_char_p(ref), C.c_void_p)
    rd.ref_len = len(ref)
    if sq is not None:
        sq = np.ascontiguousarray(sq, np.uint8)
        assert len(sq) == n
        rd.sq = sq.ctypes.data
    t = _lib.Tracks()
    col_pos = np.zeros(max(end - begin, 1), np.int64)
    with _MaxDepth(caller, max_depth):
        _lib.check(_lib.load().lfq_pileup_snv_tracks(caller.h, C.byref(rd), int(begin), int(end), int(min_plp_bq),
                                                     C.byref(t), col_pos.ctypes.data), "lfq_pileup_snv_tracks")
    return DeviceTracks(t, col_pos[: int(t.ncols)].copy())


def _pack_reads(reads, ref, lb=None, sq=None):
    n = len(reads)
    keep = {"pos": np.asarray([r["pos0"] for r in reads] or [0], np.int32)}
    cig_off = np.zeros(n + 1, np.int64)
    seq_off = np.zeros(n + 1, np.int64)
    cig, seqs, quals = [], [], []
    for i, r in enumerate(reads):
        cig.extend((l << 4) | _OPS.index(o) for o, l in r["cigar"])
        cig_off[i + 1] = len(cig)
        seqs.append(np.asarray(r["seq"], np.uint8))
        quals.append(np.asarray(r["qual"], np.uint8))
        seq_off[i + 1] = seq_off[i] + len(seqs[-1])
    keep["cig_off"], keep["seq_off"] = cig_off, seq_off
    keep["cig"] = np.asarray(cig if cig else [0], np.uint32)
    keep["seq"] = np.concatenate(seqs) if seqs else np.zeros(1, np.uint8)
    keep["qual"] = np.concatenate(quals) if quals else np.zeros(1, np.uint8)
    keep["mapq"] = np.asarray([r["mapq"] for r in reads] or [0], np.uint8)
    keep["rev"] = np.asarray([1 if r["reverse"] else 0 for r in reads] or [0], np.uint8)
    keep["ref"] = bytes(ref)
    rd = _lib.PileupReads()
    rd.n_reads = n
    rd.pos = keep["pos"].ctypes.data
    rd.cigar_off = cig_off.ctypes.data
    rd.cigar = keep["cig"].ctypes.data
    rd.seq_off = seq_off.ctypes.data
    rd.seq = keep["seq"].ctypes.data
    rd.qual = keep["qual"].ctypes.data
    rd.mapq = keep["mapq"].ctypes.data
    rd.reverse = keep["rev"].ctypes.data
    rd.ref = C.cast(C.c_char_p(keep["ref"]), C.c_void_p)
    rd.ref_len = len(keep["ref"])
    return rd, keep


def pileup_indel_columns(caller, reads, ref, begin, end, min_plp_idq=0, max_depth=None):
    """The indel fields of the pileup (`lfq_pileup_indel_columns`).  reads: as for pileup_snv_tracks, plus the
    optional per-read entries "bi", "bd", "ai", "ad" (tag bytes, uint8 arrays of the read's length, or None) and
    "sq" (int); max_depth as for pileup_snv_tracks.  -> (IndelColumns for call_indels / format_indel_record, positions of the columns)"""
    from .indel import IndelColumns, _I32
    n = len(reads)
    rd, keep = _pack_reads(reads, ref)
    n_bases = int(keep["seq_off"][-1])
    tags = _lib.PileupIndelTags()
    flags = np.zeros(max(n, 1), np.uint8)
    for bit, name in enumerate(("bi", "bd", "ai", "ad")):
        if any(r.get(name) is not None for r in reads):
            arr = np.full(max(n_bases, 1), 33, np.uint8)
            for i, r in enumerate(reads):
                if r.get(name) is not None:
                    arr[keep["seq_off"][i]:keep["seq_off"][i + 1]] = np.asarray(r[name], np.uint8)
                    flags[i] |= 1 << bit
            keep[name] = arr
            setattr(tags, name, arr.ctypes.data)
    keep["flags"] = flags
    tags.tag_flags = flags.ctypes.data
    if any(r.get("sq") is not None for r in reads):
        keep["sq"] = np.asarray([(-1 if r.get("sq") is None else r["sq"]) for r in reads], np.int32)
        tags.sq = keep["sq"].ctypes.data
    out = C.POINTER(_lib.IndelColumnsC)()
    col_pos = np.zeros(max(end - begin, 1), np.int64)
    with _MaxDepth(caller, max_depth):
        _lib.check(_lib.load().lfq_pileup_indel_columns(caller.h, C.byref(rd), C.byref(tags), int(begin), int(end),
                                                        int(min_plp_idq), C.byref(out), col_pos.ctypes.data),
                   "lfq_pileup_indel_columns")
    return _indel_columns_from_c(out, col_pos, caller)


def _indel_columns_from_c(out, col_pos, caller=None):
    """copy a context-owned lfq_indel_columns into an IndelColumns; with `caller`, remember the original so that
    call_indels can hand it back (its quality arrays are still resident on the device)"""
    from .indel import IndelColumns, _I32
    cs = out.contents
    ncols = int(cs.ncols)

    def arr(ptr, count, dt):
        if count == 0 or not ptr:
            return np.zeros(0, dt)
        return np.frombuffer(C.string_at(ptr, count * np.dtype(dt).itemsize), dtype=dt).copy()

    o = IndelColumns()
    o.ncols = ncols
    o.ref_base = arr(cs.ref_base, ncols, np.uint8)
    for name in _I32:
        setattr(o, name, arr(getattr(cs, name), ncols, np.int32))
    for sd in range(2):
        S = cs.side[sd]
        ne_off = arr(S.ne_off, ncols + 1, np.int64)
        ev_off = arr(S.ev_off, ncols + 1, np.int64)
        nev = int(ev_off[-1]) if ncols else 0
        key_off = arr(S.key_off, nev + 1, np.int64)
        rd_off = arr(S.rd_off, nev + 1, np.int64)
        nrd = int(rd_off[-1]) if nev else 0
        nne = int(ne_off[-1]) if ncols else 0
        key_chars = arr(S.key_chars, (int(key_off[-1]) if nev else 0) + 1, np.uint8)
        o.sides[sd] = {
            "non_fw": arr(S.non_fw, ncols, np.int32), "non_rv": arr(S.non_rv, ncols, np.int32), "ne_off": ne_off,
            "ne_q": arr(S.ne_q, nne, np.int16), "ne_mq": arr(S.ne_mq, nne, np.int16), "ev_off": ev_off,
            "key_off": key_off, "key_chars": key_chars, "ev_fw": arr(S.ev_fw, nev, np.int32),
            "ev_rv": arr(S.ev_rv, nev, np.int32), "rd_off": rd_off, "rd_q": arr(S.rd_q, nrd, np.int16),
            "rd_aq": arr(S.rd_aq, nrd, np.int16), "rd_mq": arr(S.rd_mq, nrd, np.int16),
            "rd_sq": arr(S.rd_sq, nrd, np.int16)}
        kc = key_chars.tobytes()
        o.keys[sd] = [kc[key_off[e]:key_off[e + 1]].decode() for e in range(nev)]
    o.cons_indel = arr(cs.cons_indel, ncols, np.uint8)
    if caller is not None:
        caller._indel_gen = getattr(caller, "_indel_gen", 0) + 1
        o._c_ptr, o._c_gen, o._c_caller = out, caller._indel_gen, caller      # valid until the context's next indel pileup
    return o, col_pos[:ncols].copy()

def skip_snv_columns(caller, skip):
    """call_vars' gate (lofreq_call.c:928-931): take the columns with skip[col] != 0 (IndelColumns.cons_indel) out of
    the SNV tracks last returned by pileup_snv_tracks"""
    skip = np.ascontiguousarray(skip, np.uint8)
    _lib.check(_lib.load().lfq_pileup_skip_snv_columns(caller.h, skip.ctypes.data, len(skip)),
               "lfq_pileup_skip_snv_columns")


class PlpSummary:
    """The header fields of `lofreq plpsummary` for the columns of a region (`lfq_plp_summary`, copied): col_pos, ref_base, fw /
    rv ([ncols, 5]: A, C, G, T, N), num_heads, num_tails, num_ins, num_dels, hrun, coverage_plp, cons_kind (0 base, 1 '+', 2
    '-') as numpy arrays and cons, the list of the columns' consensus strings as plp_summary prints them"""

    def __init__(self, ptr):
        cs = ptr.contents
        n = self.ncols = int(cs.ncols)

        def arr(p, count, dt):
            if count == 0 or not p:
                return np.zeros(0, dt)
            return np.frombuffer(C.string_at(p, count * np.dtype(dt).itemsize), dtype=dt).copy()

        self.col_pos = arr(cs.col_pos, n, np.int64)
        self.ref_base = arr(cs.ref_base, n, np.uint8)
        self.fw = arr(cs.fw, n * 5, np.int32).reshape(n, 5)
        self.rv = arr(cs.rv, n * 5, np.int32).reshape(n, 5)
        for name in ("num_heads", "num_tails", "num_ins", "num_dels", "hrun", "coverage_plp"):
            setattr(self, name, arr(getattr(cs, name), n, np.int32))
        self.cons_kind = arr(cs.cons_kind, n, np.uint8)
        self.cons_nt = arr(cs.cons_nt, n, np.uint8)
        self.cons_key_off = arr(cs.cons_key_off, n + 1, np.int64) if n else np.zeros(1, np.int64)
        self.cons_key_chars = arr(cs.cons_key_chars, int(self.cons_key_off[-1]) + 1, np.uint8)
        keys = self.cons_key_chars.tobytes()
        self.cons = [(chr(self.cons_nt[i]) if self.cons_kind[i] == 0 else
                      "+-"[self.cons_kind[i] - 1] + keys[self.cons_key_off[i]:self.cons_key_off[i + 1]].decode())
                     for i in range(n)]

    def _as_c(self):
        """an lfq_plp_summary over this object's arrays (kept alive by the returned tuple)"""
        keep = [np.ascontiguousarray(a) for a in (self.col_pos, self.ref_base, self.fw, self.rv, self.num_heads, self.num_tails,
                                                  self.num_ins, self.num_dels, self.hrun, self.coverage_plp, self.cons_kind,
                                                  self.cons_nt, self.cons_key_off, self.cons_key_chars)]
        cs = _lib.PlpSummaryC()
        cs.ncols = self.ncols
        for (name, _), a in zip(_lib.PlpSummaryC._fields_[1:], keep):
            setattr(cs, name, a.ctypes.data)
        return cs, keep


def format_plp_summary(chrom, summary):
    """`lfq_format_plp_summary` for every column of a PlpSummary -> list of the header lines of plp_summary (lofreq_call.c:
    445-459), each with its newline"""
    L = _lib.load()
    cs, _keep = summary._as_c()
    chrom = chrom if isinstance(chrom, bytes) else str(chrom).encode()
    buf = C.create_string_buffer(len(chrom) + 2048)
    lines = []
    for col in range(summary.ncols):
        n = L.lfq_format_plp_summary(buf, len(buf), chrom, C.byref(cs), col)
        _lib.check(min(n, 0), "lfq_format_plp_summary")
        lines.append(buf.raw[:n].decode())
    return lines


class PlpQuals:
    """The grouped quality bytes of `lfq_plp_quals_from_tracks` for the columns [col_begin, col_begin + ncols) of SNV tracks
    (copied): nt_off ([5 * ncols + 1]; group (column i, nucleotide k of A, C, G, T, N) = [nt_off[5i + k], nt_off[5i + k + 1])),
    bq, mq and, where the tracks have them, baq and sq (else None), in the tracks' encoding"""

    def __init__(self, ptr=None):
        self.ncols, self.col_begin = 0, 0
        self.nt_off = np.zeros(1, np.int64)
        self.bq = self.mq = np.zeros(0, np.uint8)
        self.baq = self.sq = None
        if ptr is None:
            return
        cs = ptr.contents
        self.ncols, self.col_begin = int(cs.ncols), int(cs.col_begin)
        self.nt_off = np.frombuffer(C.string_at(cs.nt_off, (5 * self.ncols + 1) * 8), dtype=np.int64).copy()
        n = int(self.nt_off[-1])

        def arr(p):
            if not p:
                return None
            return np.frombuffer(C.string_at(p, n), dtype=np.uint8).copy() if n else np.zeros(0, np.uint8)

        self.bq, self.baq, self.mq, self.sq = arr(cs.bq), arr(cs.baq), arr(cs.mq), arr(cs.sq)

    def _as_c(self):
        """an lfq_plp_quals over this object's arrays (kept alive by the returned tuple)"""
        cs = _lib.PlpQualsC()
        cs.ncols, cs.col_begin = self.ncols, self.col_begin
        keep = []
        for name in ("nt_off", "bq", "baq", "mq", "sq"):
            a = getattr(self, name)
            if a is not None:
                a = np.ascontiguousarray(a, np.int64 if name == "nt_off" else np.uint8)
                if len(a) == 0:
                    a = np.zeros(1, a.dtype)            # (an empty group list is still "present")
                keep.append(a)
                setattr(cs, name, a.ctypes.data)
        return cs, keep


def plp_quals(caller, tracks, col_begin=0, col_end=None):
    """`lfq_plp_quals_from_tracks`: the bq / baq / mq / sq bytes of the columns [col_begin, col_end) of SNV tracks grouped by
    nucleotide.  tracks: DeviceTracks with byte nt (SnvCaller.set_pileup_nt_packed(False), or those of pileup_sites), or a host
    PileupBatch / anything with _tracks() and on_device.  -> PlpQuals"""
    t = tracks._tracks()
    if col_end is None:
        col_end = int(t.ncols)
    out = C.POINTER(_lib.PlpQualsC)()
    _lib.check(_lib.load().lfq_plp_quals_from_tracks(caller.h, C.byref(t), 1 if tracks.on_device else 0, int(col_begin),
                                                     int(col_end), C.byref(out)), "lfq_plp_quals_from_tracks")
    return PlpQuals(out)


def last_plp_quals_times(caller):
    """lfq_last_plp_quals_times of the caller's context -> _lib.PlpQualsTimes"""
    t = _lib.PlpQualsTimes()
    _lib.check(_lib.load().lfq_last_plp_quals_times(caller.h, C.byref(t)), "lfq_last_plp_quals_times")
    return t


def last_bam_decode_times(caller):
    """lfq_last_bam_decode_times -> dict(upload_ms, kernels_ms, download_ms, n_reads, n_bases, n_data_bytes, n_launches)"""
    t = _lib.BamDecodeTimes()
    _lib.check(_lib.load().lfq_last_bam_decode_times(caller.h, C.byref(t)), "lfq_last_bam_decode_times")
    return {k: getattr(t, k) for k, _ in _lib.BamDecodeTimes._fields_}


def last_baq_fill_stats(caller):
    """lfq_last_baq_fill_stats -> dict(n_reads, n_need_hmm, n_stored_lb, n_stored_ai, n_stored_ad, n_hmm_launches, ms_hmm, ms_merge)"""
    t = _lib.BaqFillStats()
    _lib.check(_lib.load().lfq_last_baq_fill_stats(caller.h, C.byref(t)), "lfq_last_baq_fill_stats")
    return {k: getattr(t, k) for k, _ in _lib.BaqFillStats._fields_ if k != "pad"}


def last_bam_encode_times(caller):
    """lfq_last_bam_encode_times -> dict(upload_ms, kernels_ms, download_ms, n_reads, n_in_bytes, n_out_bytes, n_launches)"""
    t = _lib.BamEncodeTimes()
    _lib.check(_lib.load().lfq_last_bam_encode_times(caller.h, C.byref(t)), "lfq_last_bam_encode_times")
    return {k: getattr(t, k) for k, _ in _lib.BamEncodeTimes._fields_}


class BgzfError(RuntimeError):
    """lfq_bgzf_inflate found a block it cannot inflate: .status (int32 per block, nonzero = what is wrong, include/lofreq_amd.h),
    .data / .data_off as bgzf_inflate returns them (the bytes of the blocks with status 0 are intact)"""

    def __init__(self, msg, data, data_off, status):
        RuntimeError.__init__(self, msg)
        self.data, self.data_off, self.status = data, data_off, status


def _as_u8(buf):
    return np.ascontiguousarray(np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else buf, np.uint8)


def bgzf_inflate(caller, comp):
    """lfq_bgzf_inflate: the BGZF blocks `comp` (bytes or uint8 array, as they lie in the file) inflated and CRC-checked on the
    device -> (data: uint8 array, data_off: int64 [n_blocks + 1], status: int32 [n_blocks]), copies.  Raises RuntimeError for
    framing the host refuses, BgzfError (with the three arrays) when a block's status is nonzero."""
    a = _as_u8(comp)
    out = C.POINTER(_lib.BgzfResult)()
    rc = _lib.load().lfq_bgzf_inflate(caller.h, a.ctypes.data if len(a) else None, len(a), C.byref(out))
    if not out:
        _lib.check(rc, "lfq_bgzf_inflate")
    r = out.contents
    nb = int(r.n_blocks)
    data_off = np.ctypeslib.as_array(C.cast(r.data_off, C.POINTER(C.c_int64)), (nb + 1,)).copy()
    status = np.ctypeslib.as_array(C.cast(r.status, C.POINTER(C.c_int32)), (nb,)).copy() if nb else np.zeros(0, np.int32)
    data = np.ctypeslib.as_array(C.cast(r.data, C.POINTER(C.c_uint8)), (int(r.n_bytes),)).copy() if r.n_bytes else np.zeros(0, np.uint8)
    if rc != _lib.LFQ_OK:
        raise BgzfError("lfq_bgzf_inflate failed: %s (%d); status of the blocks: %s"
                        % (_lib.load().lfq_strerror(rc).decode(), rc, status.tolist()), data, data_off, status)
    return data, data_off, status


def last_bgzf_times(caller):
    """lfq_last_bgzf_times -> dict(upload_ms, kernels_ms, download_ms, n_blocks, n_in_bytes, n_out_bytes, n_launches,
    n_decodes_from_device)"""
    t = _lib.BgzfTimes()
    _lib.check(_lib.load().lfq_last_bgzf_times(caller.h, C.byref(t)), "lfq_last_bgzf_times")
    return {k: getattr(t, k) for k, _ in _lib.BgzfTimes._fields_}


def bgzf_deflate(caller, data, cuts=None, eof=False):
    """lfq_bgzf_deflate: `data` (bytes or uint8 array) cut into BGZF blocks -- every 65280 bytes, or at the offsets `cuts` -- and
    compressed on the device -> (comp: uint8 array, the blocks and, with eof, the end-of-file marker; comp_off: int64
    [n_blocks + 1]; data_off: int64 [n_blocks + 1]; btype: uint8 [n_blocks], 0 stored / 1 fixed / 2 dynamic), copies"""
    a = _as_u8(data)
    cu = None if cuts is None else np.ascontiguousarray(cuts, np.int64)
    out = C.POINTER(_lib.BgzfDeflated)()
    _lib.check(_lib.load().lfq_bgzf_deflate(caller.h, a.ctypes.data if len(a) else None, len(a),
                                            cu.ctypes.data if cu is not None and len(cu) else None, len(cu) if cu is not None else 0,
                                            _lib.LFQ_BGZF_PUT_EOF if eof else 0, C.byref(out)), "lfq_bgzf_deflate")
    return bgzf_deflated_arrays(out.contents)


def bgzf_deflated_arrays(r):
    """the copies bgzf_deflate returns, of an lfq_bgzf_deflated"""
    nb = int(r.n_blocks)
    comp_off = np.ctypeslib.as_array(C.cast(r.comp_off, C.POINTER(C.c_int64)), (nb + 1,)).copy()
    data_off = np.ctypeslib.as_array(C.cast(r.data_off, C.POINTER(C.c_int64)), (nb + 1,)).copy()
    btype = np.ctypeslib.as_array(C.cast(r.btype, C.POINTER(C.c_uint8)), (nb,)).copy() if nb else np.zeros(0, np.uint8)
    comp = np.ctypeslib.as_array(C.cast(r.comp, C.POINTER(C.c_uint8)), (int(r.n_bytes),)).copy() if r.n_bytes else np.zeros(0, np.uint8)
    return comp, comp_off, data_off, btype


def last_bgzf_deflate_times(caller):
    """lfq_last_bgzf_deflate_times -> dict(upload_ms, kernels_ms, download_ms, n_blocks, n_in_bytes, n_out_bytes, n_launches,
    n_from_device)"""
    t = _lib.BgzfDeflateTimes()
    _lib.check(_lib.load().lfq_last_bgzf_deflate_times(caller.h, C.byref(t)), "lfq_last_bgzf_deflate_times")
    return {k: getattr(t, k) for k, _ in _lib.BgzfDeflateTimes._fields_}


def bam_frame_encoded(caller, cores):
    """lfq_bam_frame_encoded: the body of a BAM file from the caller's last ReadSet.encode_bam result.  cores: the 32 core bytes of
    every ORIGINAL record (bytes or uint8 array of 32 n) -> (data: uint8 array; rec_off: int64 [n_reads + 1]), copies"""
    a = _as_u8(cores).reshape(-1)
    if len(a) % 32:
        raise ValueError("bam_frame_encoded: cores takes 32 bytes per record")
    out = C.POINTER(_lib.BamFramed)()
    keep = a if len(a) else np.zeros(32, np.uint8)          # (a pointer even for no cores: NULL is an error of its own)
    _lib.check(_lib.load().lfq_bam_frame_encoded(caller.h, keep.ctypes.data, len(a) // 32, C.byref(out)), "lfq_bam_frame_encoded")
    r = out.contents
    n = int(r.n_reads)
    rec_off = np.ctypeslib.as_array(C.cast(r.rec_off, C.POINTER(C.c_int64)), (n + 1,)).copy()
    data = np.ctypeslib.as_array(C.cast(r.data, C.POINTER(C.c_uint8)), (int(r.n_bytes),)).copy() if r.n_bytes else np.zeros(0, np.uint8)
    return data, rec_off


def _scan_opts(tid=-1, beg=0, end=None, min_mq=0, max_mq=255, no_orphan=False, flag_mask=None):
    o = _lib.BamScanOpts()
    _lib.load().lfq_bam_scan_opts_init(C.byref(o))
    o.tid, o.beg, o.min_mq, o.max_mq, o.no_orphan = int(tid), int(beg), int(min_mq), int(max_mq), 1 if no_orphan else 0
    if end is not None:
        o.end = int(end)
    if flag_mask is not None:
        o.flag_mask = int(flag_mask)
    return o


def bam_scan_records(bam, first=0, stop=None, **opts):
    """lfq_bam_scan_records (host only): the records of inflated BAM bytes bam[first:stop], filtered as sam_itr_next + mplp_func
    keep them.  opts: tid (-1 = any), beg, end, min_mq, max_mq, no_orphan, flag_mask (default 4 | 256 | 512 | 1024).
    -> dict: data_off [n + 1], data_end, pos, flag, mapq, l_qname, n_cigar, l_qseq [n] of the kept records (record r is
    bam[data_off[r]:data_end[r]]), n_seen, n_consumed"""
    L = _lib.load()
    a = _as_u8(bam)
    o = _scan_opts(**opts)
    out = C.POINTER(_lib.BamScan)()
    _lib.check(L.lfq_bam_scan_records(a.ctypes.data if len(a) else None, int(first), len(a) if stop is None else int(stop),
                                      C.byref(o), C.byref(out)), "lfq_bam_scan_records")
    try:
        s = out.contents
        n = int(s.recs.n_reads)
        get = lambda p, ct, k: np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), (k,)).copy() if k else np.zeros(0, ct)
        return {"data_off": get(s.recs.data_off, C.c_int64, n + 1), "data_end": get(s.data_end, C.c_int64, n),
                "pos": get(s.recs.pos, C.c_int32, n), "flag": get(s.recs.flag, C.c_uint16, n), "mapq": get(s.recs.mapq, C.c_uint8, n),
                "l_qname": get(s.recs.l_qname, C.c_uint16, n), "n_cigar": get(s.recs.n_cigar, C.c_uint32, n),
                "l_qseq": get(s.recs.l_qseq, C.c_int32, n), "n_seen": int(s.n_seen), "n_consumed": int(s.n_consumed)}
    finally:
        L.lfq_bam_scan_free(out)


def _format_grown(call, what):
    """a formatter whose text grows with the depth: ask for the length, then write"""
    n = call(None, 0)
    _lib.check(min(n, 0), what)
    buf = C.create_string_buffer(n + 1)
    m = call(buf, n + 1)
    _lib.check(min(m, 0), what)
    return buf.raw[:m].decode()


def format_plp_quals(quals, flag, cols=None):
    """`lfq_format_plp_quals` (lofreq_call.c:460-489): the nucleotide quality lines of the columns `cols` (indices of the
    tracks; default: every column of the PlpQuals) -> list of strings, one per column ('' for a column without a kept base).
    flag: LFQ_USE_BAQ / LFQ_USE_SQ decide the BAQ values and the SQ line as varcall_conf_t.flag does"""
    L = _lib.load()
    cs, _keep = quals._as_c()
    if cols is None:
        cols = range(quals.col_begin, quals.col_begin + quals.ncols)
    return [_format_grown(lambda b, n, col=col: L.lfq_format_plp_quals(b, n, C.byref(cs), int(col), int(flag)),
                          "lfq_format_plp_quals") for col in cols]


def format_plp_indel_quals(indel_cols, cols=None):
    """`lfq_format_plp_indel_quals` (lofreq_call.c:491-598): the indel quality lines and the closing empty line of the columns
    `cols` (default: all) of an IndelColumns made with SnvCaller.set_indel_arrays_all_columns(True) -> list of strings"""
    L = _lib.load()
    cs = indel_cols.c_struct()
    for sd in range(2):
        S = indel_cols.sides[sd]
        if len(S["ne_q"]) < int(S["ne_off"][-1]) or len(S["ne_mq"]) < int(S["ne_off"][-1]):
            cs.side[sd].ne_q = None                     # device-only arrays (set_indel_arrays_on_host(False))
            cs.side[sd].ne_mq = None
    if cols is None:
        cols = range(indel_cols.ncols)
    return [_format_grown(lambda b, n, col=col: L.lfq_format_plp_indel_quals(b, n, C.byref(cs), int(col)),
                          "lfq_format_plp_indel_quals") for col in cols]


class ReadSet:
    """The reads of one contig region resident on the device (`lfq_readset`): upload once, then BAQ / IDAQ, source
    quality, both pileups and the calls without the per-base arrays leaving HBM.

        rs = ReadSet(caller, reads, ref)          # reads: dicts as for pileup_snv_tracks (+ "bi", "bd")
        rs.baq(idaq=True); rs.source_qual()       # optional steps, results stay resident
        tracks = rs.pileup_snv(0, len(ref)); cols, col_pos = rs.pileup_indels(0, len(ref))
    """

    def __init__(self, caller, reads, ref):
        self.caller = caller
        self.L = _lib.load()
        n = len(reads)
        self.n = n
        rd, keep = _pack_reads(reads, ref)
        n_bases = int(keep["seq_off"][-1])
        tags = _lib.PileupIndelTags()
        flags = np.zeros(max(n, 1), np.uint8)
        for bit, name in enumerate(("bi", "bd", "ai", "ad")):
            if any(r.get(name) is not None for r in reads):
                arr = np.full(max(n_bases, 1), 33, np.uint8)
                for i, r in enumerate(reads):
                    if r.get(name) is not None:
                        arr[keep["seq_off"][i]:keep["seq_off"][i + 1]] = np.asarray(r[name], np.uint8)
                        flags[i] |= 1 << bit
                keep[name] = arr
                setattr(tags, name, arr.ctypes.data)
        keep["flags"] = flags
        tags.tag_flags = flags.ctypes.data
        if any(r.get("lb") is not None for r in reads):
            keep["lb"] = np.concatenate([np.asarray(r["lb"], np.uint8) for r in reads])
            rd.baq = keep["lb"].ctypes.data
        self._keep = keep                           # the host arrays must outlive the read set
        self.seq_off = keep["seq_off"]
        h = C.c_void_p()
        _lib.check(self.L.lfq_readset_create(caller.h, C.byref(rd), C.byref(tags), C.byref(h)), "lfq_readset_create")
        self.h = h
        if not hasattr(caller, "_readsets"):
            import weakref
            caller._readsets = weakref.WeakSet()
        caller._readsets.add(self)                  # SnvCaller.close() closes its read sets first

    @classmethod
    def from_arrays(cls, caller, R):
        """the same from flat arrays (no per-read Python objects): R = dict with n, pos (int32), cig_off / seq_off (int64),
        cig (uint32, BAM encoding), seq (codes 0..4), qual, mapq, rev (uint8 per read), ref (bytes), and optionally
        bi / bd (tag bytes per base), lb (tag bytes per base), flags (uint8 per read, bits 0 / 1 = has BI / BD)"""
        self = cls.__new__(cls)
        self.caller = caller
        self.L = _lib.load()
        self.n = int(R["n"])
        keep = {k: np.ascontiguousarray(R[k], dt) for k, dt in (("pos", np.int32), ("cig_off", np.int64), ("cig", np.uint32),
                                                                ("seq_off", np.int64), ("seq", np.uint8), ("qual", np.uint8),
                                                                ("mapq", np.uint8), ("rev", np.uint8))}
        keep["ref"] = bytes(R["ref"])
        rd = _lib.PileupReads()
        rd.n_reads = self.n
        rd.pos, rd.cigar_off, rd.cigar = keep["pos"].ctypes.data, keep["cig_off"].ctypes.data, keep["cig"].ctypes.data
        rd.seq_off, rd.seq, rd.qual = keep["seq_off"].ctypes.data, keep["seq"].ctypes.data, keep["qual"].ctypes.data
        rd.mapq, rd.reverse = keep["mapq"].ctypes.data, keep["rev"].ctypes.data
        rd.ref = C.cast(C.c_char_p(keep["ref"]), C.c_void_p)
        rd.ref_len = len(keep["ref"])
        if hasattr(R["ref"], "seq_ptr"):            # a fasta.Contig: its own pointer, which the library recognises and hands over
            keep["contig"] = R["ref"]               # on the device; it must stay the file's live fetch result while the read set lives
            rd.ref = C.c_void_p(R["ref"].seq_ptr)
        if R.get("lb") is not None:
            keep["lb"] = np.ascontiguousarray(R["lb"], np.uint8)
            rd.baq = keep["lb"].ctypes.data
        tags = _lib.PileupIndelTags()
        for name in ("bi", "bd"):
            if R.get(name) is not None:
                keep[name] = np.ascontiguousarray(R[name], np.uint8)
                setattr(tags, name, keep[name].ctypes.data)
        if R.get("flags") is not None:
            keep["flags"] = np.ascontiguousarray(R["flags"], np.uint8)
            tags.tag_flags = keep["flags"].ctypes.data
        self._keep = keep
        self.seq_off = keep["seq_off"]
        h = C.c_void_p()
        _lib.check(self.L.lfq_readset_create(caller.h, C.byref(rd), C.byref(tags), C.byref(h)), "lfq_readset_create")
        self.h = h
        if not hasattr(caller, "_readsets"):
            import weakref
            caller._readsets = weakref.WeakSet()
        caller._readsets.add(self)
        return self

    @classmethod
    def from_bam_records(cls, caller, data, data_off, pos, flag, mapq, l_qname, n_cigar, l_qseq, ref, read_tags=0):
        """lfq_readset_create_from_bam: the read set of BAM records as they lie in memory -- data: the bytes of every record from
        read_name on (bam1_t.data), concatenated; data_off [n + 1] into it; pos, flag, mapq, l_qname, n_cigar, l_qseq: the core
        fields per read; ref: the contig (bytes).  Bases, qualities and BI / BD are decoded on the device; the read set owns
        its host arrays, so only `ref` is kept alive here.  read_tags (lfq_readset_create_from_bam_tags): LFQ_BAM_READ_LB /
        LFQ_BAM_READ_IDAQ keep the first lb / ai and ad field of every record on the device for baq_fill()."""
        self = cls.__new__(cls)
        self.caller = caller
        self.L = _lib.load()
        a = {k: np.ascontiguousarray(v, dt) for k, v, dt in (
            ("data", data, np.uint8), ("data_off", data_off, np.int64), ("pos", pos, np.int32), ("flag", flag, np.uint16),
            ("mapq", mapq, np.uint8), ("l_qname", l_qname, np.uint16), ("n_cigar", n_cigar, np.uint32), ("l_qseq", l_qseq, np.int32))}
        self.n = len(a["pos"])
        if len(a["data_off"]) != self.n + 1 or any(len(a[k]) != self.n for k in ("flag", "mapq", "l_qname", "n_cigar", "l_qseq")):
            raise ValueError("from_bam_records: data_off takes n + 1 entries, every other per-read array n")
        rc = _lib.BamRecords()
        rc.n_reads = self.n
        for k in a:
            setattr(rc, k, a[k].ctypes.data)
        self._keep = {"ref": bytes(ref)}
        rc.ref = C.cast(C.c_char_p(self._keep["ref"]), C.c_void_p)
        rc.ref_len = len(self._keep["ref"])
        self.seq_off = np.concatenate([[0], np.cumsum(a["l_qseq"], dtype=np.int64)]).astype(np.int64)
        h = C.c_void_p()
        if read_tags:
            _lib.check(self.L.lfq_readset_create_from_bam_tags(caller.h, C.byref(rc), int(read_tags), C.byref(h)),
                       "lfq_readset_create_from_bam_tags")
        else:
            _lib.check(self.L.lfq_readset_create_from_bam(caller.h, C.byref(rc), C.byref(h)), "lfq_readset_create_from_bam")
        self.h = h
        if not hasattr(caller, "_readsets"):
            import weakref
            caller._readsets = weakref.WeakSet()
        caller._readsets.add(self)
        return self

    @classmethod
    def from_bgzf(cls, caller, comp, first, ref, stop=-1, read_tags=0, **opts):
        """lfq_readset_create_from_bgzf: the read set of the BAM records in the BGZF blocks `comp` (bytes or uint8 array) --
        inflated on the device, scanned from byte `first` of the inflated data to `stop` (negative: its end) under `opts`
        (bam_scan_records), decoded from the device copy.  .n_consumed: the scan's; .kept: the dict bam_scan_records returns.
        (To know the kept reads on this side the binding inflates and scans once more in front of the call.)"""
        self = cls.__new__(cls)
        self.caller = caller
        self.L = _lib.load()
        a = _as_u8(comp)
        data, _, _ = bgzf_inflate(caller, a)
        self.kept = bam_scan_records(data, int(first), None if stop < 0 else int(stop), **opts)
        self.n = len(self.kept["pos"])
        self.seq_off = np.concatenate([[0], np.cumsum(self.kept["l_qseq"], dtype=np.int64)]).astype(np.int64)
        self._keep = {"ref": bytes(ref)}
        o = _scan_opts(**opts)
        h = C.c_void_p()
        consumed = C.c_int64(0)
        _lib.check(self.L.lfq_readset_create_from_bgzf(caller.h, a.ctypes.data if len(a) else None, len(a), int(first), int(stop),
                                                       C.byref(o), C.cast(C.c_char_p(self._keep["ref"]), C.c_void_p),
                                                       len(self._keep["ref"]), int(read_tags), C.byref(h), C.byref(consumed)),
                   "lfq_readset_create_from_bgzf")
        self.n_consumed = int(consumed.value)
        self.h = h
        if not hasattr(caller, "_readsets"):
            import weakref
            caller._readsets = weakref.WeakSet()
        caller._readsets.add(self)
        return self

    def fetch_bases(self):
        """lfq_readset_fetch_bases: the resident per-base inputs read back from the device -> (seq codes 0..15, qual, bi, bd:
        uint8 per base in the seq_off layout, '!' throughout for a tag array the read set lacks; flags: uint8 per read, bit 0 / 1
        = has BI / BD)"""
        nb = int(self.seq_off[-1])
        out = [np.zeros(max(nb, 1), np.uint8) for _ in range(4)] + [np.zeros(max(self.n, 1), np.uint8)]
        _lib.check(self.L.lfq_readset_fetch_bases(self.caller.h, self.h, *[o.ctypes.data for o in out]), "lfq_readset_fetch_bases")
        return tuple(o[:nb] for o in out[:4]) + (out[4][: self.n],)

    def fetch_stored_tags(self):
        """lfq_readset_fetch_stored_tags: the lb / ai / ad strings the records carried, from the device -> (lb, ai, ad: uint8 per
        base in the seq_off layout, '!' throughout for a read without the tag; flags: uint8 per read, bit 0 / 1 / 2 = lb / ai /
        ad stored)"""
        nb = int(self.seq_off[-1])
        out = [np.zeros(max(nb, 1), np.uint8) for _ in range(3)] + [np.zeros(max(self.n, 1), np.uint8)]
        _lib.check(self.L.lfq_readset_fetch_stored_tags(self.caller.h, self.h, *[o.ctypes.data for o in out]),
                   "lfq_readset_fetch_stored_tags")
        return tuple(o[:nb] for o in out[:3]) + (out[3][: self.n],)

    def encode_bam(self, recs, src=None, what=_lib.LFQ_BAM_PUT_ALIGNMENT):
        """lfq_readset_encode_bam: the results of this read set's steps written into the bytes of the BAM records its reads came
        from, on the device.  recs: dict with the arrays from_bam_records takes (data, data_off, pos, flag, mapq, l_qname, n_cigar,
        l_qseq) -- the ORIGINAL records; src[j]: the record of this set's read j (None: the identity; after viterbi() its order);
        what: LFQ_BAM_* bits.  -> dict in the same layout, records in this set's read order: data, data_off, pos, n_cigar, src,
        and flag / mapq / l_qname / l_qseq gathered through src (+ "ref" where recs has it) -- ready for from_bam_records"""
        a = {k: np.ascontiguousarray(recs[k], dt) for k, dt in (
            ("data", np.uint8), ("data_off", np.int64), ("pos", np.int32), ("flag", np.uint16), ("mapq", np.uint8),
            ("l_qname", np.uint16), ("n_cigar", np.uint32), ("l_qseq", np.int32))}
        n = len(a["pos"])
        if len(a["data_off"]) != n + 1 or any(len(a[k]) != n for k in ("flag", "mapq", "l_qname", "n_cigar", "l_qseq")):
            raise ValueError("encode_bam: data_off takes n + 1 entries, every other per-read array n")
        if src is not None:
            src = np.ascontiguousarray(src, np.int64)
            if len(src) != n:
                raise ValueError("encode_bam: src takes n entries")
        rc = _lib.BamRecords()
        rc.n_reads = n
        for k in a:
            setattr(rc, k, a[k].ctypes.data)
        out = C.POINTER(_lib.BamEncoded)()
        _lib.check(self.L.lfq_readset_encode_bam(self.caller.h, self.h, C.byref(rc), src.ctypes.data if src is not None else None,
                                                 int(what), C.byref(out)), "lfq_readset_encode_bam")
        e = out.contents
        m = int(e.n_reads)

        def arr(p, count, dt):
            if count == 0 or not p:
                return np.zeros(0, dt)
            return np.frombuffer(C.string_at(p, count * np.dtype(dt).itemsize), dtype=dt).copy()

        off = arr(e.data_off, m + 1, np.int64) if m else np.zeros(1, np.int64)
        s = arr(e.src, m, np.int64)
        res = {"data": arr(e.data, int(off[-1]), np.uint8), "data_off": off, "pos": arr(e.pos, m, np.int32),
               "n_cigar": arr(e.n_cigar, m, np.uint32), "src": s}
        for k in ("flag", "mapq", "l_qname", "l_qseq"):
            res[k] = a[k][s]
        if "ref" in recs:
            res["ref"] = recs["ref"]
        return res

    def close(self):
        if getattr(self, "h", None):
            self.L.lfq_readset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ref_from_device(self):
        """lfq_readset_ref_from_device: the contig was copied from a live Fasta.fetch result on the device, not across the link"""
        return bool(self.L.lfq_readset_ref_from_device(self.h))

    def baq(self, extended=True, idaq=False):
        _lib.check(self.L.lfq_readset_baq(self.caller.h, self.h, 1 if extended else 0, 1 if idaq else 0), "lfq_readset_baq")

    def baq_fill(self, extended=True, idaq=False, redo_baq=False):
        """lfq_readset_baq_fill: baq() that keeps the stored lb / ai / ad of from_bam_records(..., read_tags=) and runs the HMM
        only for the reads that lack a tag (`lofreq call`'s default; redo_baq: -D)"""
        _lib.check(self.L.lfq_readset_baq_fill(self.caller.h, self.h, 1 if extended else 0, 1 if idaq else 0, 1 if redo_baq else 0),
                   "lfq_readset_baq_fill")

    def source_qual(self, def_nm_q=-1, min_bq=6, ign=None):
        sq = np.zeros(max(self.n, 1), np.int32)
        if ign is not None:
            ign = np.ascontiguousarray(ign, np.uint8)
        _lib.check(self.L.lfq_readset_source_qual(self.caller.h, self.h, int(def_nm_q), int(min_bq),
                                                  ign.ctypes.data if ign is not None else None, sq.ctypes.data),
                   "lfq_readset_source_qual")
        return sq[: self.n]

    def fetch_tags(self, idaq=False):
        nb = max(int(self.seq_off[-1]), 1)
        lb = np.zeros(nb, np.uint8)
        ai = np.zeros(nb, np.uint8) if idaq else None
        ad = np.zeros(nb, np.uint8) if idaq else None
        fl = np.zeros(max(self.n, 1), np.uint8) if idaq else None
        p = lambda a: a.ctypes.data if a is not None else None
        _lib.check(self.L.lfq_readset_fetch_tags(self.caller.h, self.h, p(lb), p(ai), p(ad), p(fl)), "lfq_readset_fetch_tags")
        return lb, ai, ad, fl

    def viterbi(self, def_qual=-1):
        """lfq_readset_viterbi (`lofreq viterbi`), before every other step: -> (a NEW ReadSet of the same reads, realigned and
        stably sorted by new position; the result as viterbi_arrays returns it, in this set's read order; order).  This set
        is not changed."""
        from .viterbi import readset_viterbi
        return readset_viterbi(self, def_qual)

    def indelqual(self, mode="dindel", ins_qual=0, del_qual=None):
        """lfq_readset_indelqual (`lofreq indelqual`): BI / BD computed on the device copy, for a read set created without"""
        from .indelqual import readset_indelqual
        readset_indelqual(self, mode, ins_qual, del_qual)

    def fetch_indelquals(self):
        from .indelqual import readset_fetch_indelquals
        return readset_fetch_indelquals(self)

    def kept_reads(self, max_depth=None):
        """lfq_readset_kept_reads: which reads the pileups take under the cap -> (uint8 mask, number kept)"""
        keep = np.zeros(max(self.n, 1), np.uint8)
        n_kept = C.c_int64(-1)
        with _MaxDepth(self.caller, max_depth):
            _lib.check(self.L.lfq_readset_kept_reads(self.caller.h, self.h, keep.ctypes.data, C.byref(n_kept)),
                       "lfq_readset_kept_reads")
        return keep[: self.n], int(n_kept.value)

    def pileup_snv(self, begin, end, min_plp_bq=3, sync=False, max_depth=None):
        """lfq_readset_pileup_snv returns when the scatter pass is queued: the tracks are complete in stream order (the calls
        that take them are queued behind); sync=True waits, for code that reads the device memory itself.  max_depth: -d
        of `lofreq call` (lfq_set_max_depth), None = no cap"""
        t = _lib.Tracks()
        col_pos = np.zeros(max(end - begin, 1), np.int64)
        with _MaxDepth(self.caller, max_depth):
            _lib.check(self.L.lfq_readset_pileup_snv(self.caller.h, self.h, int(begin), int(end), int(min_plp_bq),
                                                     C.byref(t), col_pos.ctypes.data), "lfq_readset_pileup_snv")
        if sync:
            self.caller.synchronize()
        return DeviceTracks(t, col_pos[: int(t.ncols)].copy())

    def pileup_indels(self, begin, end, min_plp_idq=0, max_depth=None):
        out = C.POINTER(_lib.IndelColumnsC)()
        col_pos = np.zeros(max(end - begin, 1), np.int64)
        with _MaxDepth(self.caller, max_depth):
            _lib.check(self.L.lfq_readset_pileup_indels(self.caller.h, self.h, int(begin), int(end), int(min_plp_idq),
                                                        C.byref(out), col_pos.ctypes.data), "lfq_readset_pileup_indels")
        return _indel_columns_from_c(out, col_pos, self.caller)

    def pileup_sites(self, pos, min_plp_bq=3):
        """lfq_readset_pileup_sites: the pileup at a LIST of positions, column i = pos[i] (any order, duplicates allowed; a
        position no read covers is an empty column).  -> (DeviceTracks with unpacked nt, valid until the context's next
        pileup_sites / uniq call; coverage_plp; num_tails)"""
        pos = np.ascontiguousarray(pos, np.int64)
        n = len(pos)
        cov = np.zeros(max(n, 1), np.int32)
        tails = np.zeros(max(n, 1), np.int32)
        t = _lib.Tracks()
        _lib.check(self.L.lfq_readset_pileup_sites(self.caller.h, self.h, pos.ctypes.data, n, int(min_plp_bq), C.byref(t),
                                                   cov.ctypes.data, tails.ctypes.data), "lfq_readset_pileup_sites")
        return DeviceTracks(t, pos.copy()), cov[:n], tails[:n]

    def uniq(self, pos, ref, alt, af, indel_key=None, use_det_lim=False, min_plp_bq=3):
        """lfq_readset_uniq (`lofreq uniq` for a list of variants on this read set, the OTHER sample's reads filtered as
        uniq's mpileup filters them).  pos: 0-based positions; ref / alt: the REF / ALT strings; af: the AF values (or
        --uni-freq); indel_key: which variants carry the INDEL key.  -> dict of arrays: coverage, alt_count, uq (-1 = no
        UQ tag), pvalue (-1.0 = none) and detectable (the UNIQ flag of --use-det-lim)"""
        n = len(pos)
        pos = np.ascontiguousarray(pos, np.int64)
        enc = lambda x: x if isinstance(x, bytes) else str(x).encode()
        refs, alts = [enc(x) for x in ref], [enc(x) for x in alt]
        assert len(refs) == n and len(alts) == n and len(af) == n
        ref_off = np.zeros(n + 1, np.int64)
        alt_off = np.zeros(n + 1, np.int64)
        ref_off[1:] = np.cumsum([len(x) for x in refs])
        alt_off[1:] = np.cumsum([len(x) for x in alts])
        ref_b, alt_b = b"".join(refs) + b"\0", b"".join(alts) + b"\0"
        af = np.ascontiguousarray(af, np.float32)
        v = _lib.UniqVariants()
        v.n = n
        v.pos, v.ref_off, v.alt_off = pos.ctypes.data, ref_off.ctypes.data, alt_off.ctypes.data
        v.ref, v.alt = C.cast(C.c_char_p(ref_b), C.c_void_p), C.cast(C.c_char_p(alt_b), C.c_void_p)
        v.af = af.ctypes.data
        if indel_key is not None:
            indel_key = np.ascontiguousarray(np.asarray(indel_key, bool), np.uint8)
            assert len(indel_key) == n
            v.indel_key_or_null = indel_key.ctypes.data
        res = {"coverage": np.zeros(max(n, 1), np.int32), "alt_count": np.zeros(max(n, 1), np.int32),
               "uq": np.zeros(max(n, 1), np.int32), "pvalue": np.zeros(max(n, 1), np.float64),
               "detectable": np.zeros(max(n, 1), np.uint8)}
        o = _lib.UniqResult()
        for k, a in res.items():
            setattr(o, k, a.ctypes.data)
        _lib.check(self.L.lfq_readset_uniq(self.caller.h, self.h, C.byref(v), 1 if use_det_lim else 0, int(min_plp_bq),
                                           C.byref(o)), "lfq_readset_uniq")
        return {k: a[:n] for k, a in res.items()}

    def plp_summary(self, begin, end, min_plp_bq=3, min_plp_idq=0, max_depth=None):
        """lfq_readset_plp_summary: the header fields of `lofreq plpsummary` for the covered positions of [begin, end), numbered as
        the columns of pileup_snv / pileup_indels -> PlpSummary.  Runs the indel pileup of the region: an IndelColumns obtained
        earlier from this caller is superseded (call_indels then packs it from its host copy), as after pileup_indels"""
        out = C.POINTER(_lib.PlpSummaryC)()
        with _MaxDepth(self.caller, max_depth):
            _lib.check(self.L.lfq_readset_plp_summary(self.caller.h, self.h, int(begin), int(end), int(min_plp_bq),
                                                      int(min_plp_idq), C.byref(out)), "lfq_readset_plp_summary")
        self.caller._indel_gen = getattr(self.caller, "_indel_gen", 0) + 1
        return PlpSummary(out)

    def plpsummary_text(self, chrom, begin, end, flag, min_plp_bq=3, min_plp_idq=0, max_depth=None):
        """The text of `lofreq plpsummary` for the covered positions of [begin, end): one string per column -- header line
        (lfq_format_plp_summary), nucleotide quality lines (lfq_plp_quals_from_tracks + lfq_format_plp_quals), indel quality
        lines and the closing empty line (lfq_format_plp_indel_quals).  flag: LFQ_USE_BAQ / LFQ_USE_SQ as varcall_conf_t.flag.
        Runs plp_summary, pileup_snv with byte nt and pileup_indels with the arrays of every column (the context offers no way
        to the lfq_indel_columns the summary call left behind, so the indel pileup runs a second time); the caller's nt layout
        and all-columns switch are set for the duration of the call and put back to their defaults (packed, off)"""
        c = self.caller
        s = self.plp_summary(begin, end, min_plp_bq=min_plp_bq, min_plp_idq=min_plp_idq, max_depth=max_depth)
        heads = format_plp_summary(chrom, s)
        c.set_pileup_nt_packed(False)
        c.set_indel_arrays_all_columns(True)
        try:
            t = self.pileup_snv(begin, end, min_plp_bq=min_plp_bq, max_depth=max_depth)
            q = plp_quals(c, t, 0, t.ncols)
            cols, col_pos = self.pileup_indels(begin, end, min_plp_idq=min_plp_idq, max_depth=max_depth)
        finally:
            c.set_pileup_nt_packed(True)
            c.set_indel_arrays_all_columns(False)
        if not (t.ncols == cols.ncols == s.ncols and t.col_pos.tolist() == col_pos.tolist() == s.col_pos.tolist()):
            raise RuntimeError("plpsummary_text: the three pileups disagree on the columns")
        nts = format_plp_quals(q, flag)
        ind = format_plp_indel_quals(cols)
        return [h + a + b for h, a, b in zip(heads, nts, ind)]

    def last_summary_times(self):
        """lfq_last_summary_times of the caller's context -> _lib.SummaryTimes"""
        t = _lib.SummaryTimes()
        _lib.check(self.L.lfq_last_summary_times(self.caller.h, C.byref(t)), "lfq_last_summary_times")
        return t

    def last_sites_times(self):
        """lfq_last_sites_times of the caller's context -> _lib.SitesTimes"""
        t = _lib.SitesTimes()
        _lib.check(self.L.lfq_last_sites_times(self.caller.h, C.byref(t)), "lfq_last_sites_times")
        return t
