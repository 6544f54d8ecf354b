"""Host mirror of `lofreq viterbi` (fetch_func, lofreq_viterbi.c:107-345; viterbi and left_align_indels, viterbi.c): a batch
of mapped reads of one contig -> their position and CIGAR after the realignment of the reads with an indel, through
`lfq_viterbi_batch`."""
import ctypes as C

import numpy as np

from . import _lib
from .baq import _OPS

NO_INDEL, SKIPPED_OP, ALL_Q2, REALIGNED = (_lib.LFQ_VIT_NO_INDEL, _lib.LFQ_VIT_SKIPPED_OP, _lib.LFQ_VIT_ALL_Q2,
                                           _lib.LFQ_VIT_REALIGNED)
STATUS_MASK, CHANGED = _lib.LFQ_VIT_STATUS_MASK, _lib.LFQ_VIT_CHANGED


def pack_reads(reads, ref):
    """the read dicts of baq_batch -> (lfq_baq_reads, the arrays it points into)"""
    n = len(reads)
    pos = np.asarray([r["pos0"] for r in reads], np.int32).reshape(n)
    cig_n = np.asarray([len(r["cigar"]) for r in reads], np.int64).reshape(n)
    seq_n = np.asarray([len(r["seq"]) for r in reads], np.int64).reshape(n)
    cig_off = np.zeros(n + 1, np.int64)
    seq_off = np.zeros(n + 1, np.int64)
    np.cumsum(cig_n, out=cig_off[1:])
    np.cumsum(seq_n, out=seq_off[1:])
    cig = np.asarray([(l << 4) | _OPS.index(o) for r in reads for o, l in r["cigar"]] or [0], np.uint32)
    seq = np.concatenate([np.asarray(r["seq"], np.uint8) for r in reads]) if n and seq_off[-1] else np.zeros(1, np.uint8)
    qual = np.concatenate([np.asarray(r["qual"], np.uint8) for r in reads]) if n and seq_off[-1] else np.zeros(1, np.uint8)
    ref = bytes(ref)
    rd = _lib.BaqReads()
    rd.n_reads = n
    rd.pos = pos.ctypes.data
    rd.cigar_off = cig_off.ctypes.data
    rd.cigar = cig.ctypes.data
    rd.seq_off = seq_off.ctypes.data
    rd.seq = seq.ctypes.data
    rd.qual = qual.ctypes.data
    rd.ref = C.cast(C.c_char_p(ref), C.c_void_p)
    rd.ref_len = len(ref)
    return rd, (pos, cig_off, seq_off, cig, seq, qual, ref)


def result_arrays(res):
    """copies of a context-owned lfq_viterbi_result: (pos [n], status [n], cigar_off [n + 1], cigar)"""
    r = res.contents
    n = int(r.n_reads)

    def arr(ptr, count, dtype):
        if count == 0:
            return np.zeros(0, dtype)
        return np.frombuffer((C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr), dtype).copy()
    cig_off = arr(r.cigar_off, n + 1, np.int64)
    return arr(r.pos, n, np.int32), arr(r.status, n, np.uint8), cig_off, arr(r.cigar, int(cig_off[-1]), np.uint32)


def viterbi_arrays(caller, rd, def_qual=-1):
    """lfq_viterbi_batch on a packed batch -> copies of (pos [n], status [n], cigar_off [n + 1], cigar)"""
    res = C.POINTER(_lib.ViterbiResult)()
    _lib.check(_lib.load().lfq_viterbi_batch(caller.h, C.byref(rd), int(def_qual), C.byref(res)), "lfq_viterbi_batch")
    return result_arrays(res)


def readset_viterbi(rs, def_qual=-1):
    """lfq_readset_viterbi: the reads of a resident ReadSet realigned into a NEW ReadSet, stably sorted by new position; `rs`
    stays as it is.  -> (the new ReadSet, the result in the form viterbi_arrays returns and in the INPUT read order, order:
    int64 [n], order[j] = input index of the read at place j of the new set)"""
    res = C.POINTER(_lib.ViterbiResult)()
    h, order_p = C.c_void_p(), C.c_void_p()
    _lib.check(rs.L.lfq_readset_viterbi(rs.caller.h, rs.h, int(def_qual), C.byref(h), C.byref(res), C.byref(order_p)),
               "lfq_readset_viterbi")
    result = result_arrays(res)
    n = rs.n
    order = (np.frombuffer((C.c_char * (n * 8)).from_address(order_p.value), np.int64).copy() if n else np.zeros(0, np.int64))
    new = type(rs).__new__(type(rs))
    new.caller, new.L, new.n, new.h = rs.caller, rs.L, n, h
    new._keep = {}                                  # the new read set owns its host arrays
    lens = np.diff(np.asarray(rs.seq_off, np.int64))[:n]
    new.seq_off = np.concatenate([[0], np.cumsum(lens[order])]).astype(np.int64)
    rs.caller._readsets.add(new)
    return new, result, order


def viterbi_batch(caller, reads, ref, def_qual=-1):
    """reads: list of dicts {pos0, cigar [(op, len)], seq (base codes), qual (phred)} of mapped reads of one contig; ref: the
    contig (bytes); def_qual: -q / --defqual (negative: the median quality of the read stands in for a quality of 2).
    -> per read (pos0, cigar [(op, len)], status): status & STATUS_MASK is NO_INDEL, SKIPPED_OP, ALL_Q2 (read left as it is)
    or REALIGNED, with the CHANGED bit where position or CIGAR differ from the input.  The output is not sorted by position."""
    rd, keep = pack_reads(reads, ref)
    pos, status, cig_off, cig = viterbi_arrays(caller, rd, def_qual)
    del keep
    return [(int(pos[i]), [(_OPS[int(w) & 15], int(w) >> 4) for w in cig[cig_off[i]:cig_off[i + 1]]], int(status[i]))
            for i in range(len(reads))]


def last_times(caller):
    """device time of the realignment kernels of the caller's last viterbi_batch, their launches, reads and realigned reads"""
    t = _lib.ViterbiTimes()
    _lib.check(_lib.load().lfq_last_viterbi_times(caller.h, C.byref(t)), "lfq_last_viterbi_times")
    return {"ms_kernels": float(t.ms_kernels), "n_launches": int(t.n_launches), "n_reads": int(t.n_reads),
            "n_realigned": int(t.n_realigned)}
