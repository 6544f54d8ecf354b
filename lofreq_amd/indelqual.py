"""Host mirror of `lofreq indelqual` (lofreq_indelqual.c): the BI / BD per-base indel qualities of a batch of mapped reads of
one contig through `lfq_indelqual_batch`, and the same as a step of a resident read set (`lfq_readset_indelqual`)."""
import ctypes as C

import numpy as np

from . import _lib
from .viterbi import pack_reads

UNIFORM, DINDEL = _lib.LFQ_IDQ_UNIFORM, _lib.LFQ_IDQ_DINDEL


def make_conf(mode="dindel", ins_qual=0, del_qual=None):
    """mode: "dindel" (--dindel), "uniform" (-u INT[,INT]) or an LFQ_IDQ_* value; one quality given sets both"""
    conf = _lib.IndelqualConf()
    conf.mode = {"dindel": DINDEL, "uniform": UNIFORM}.get(mode, mode)
    conf.ins_qual = int(ins_qual)
    conf.del_qual = int(ins_qual if del_qual is None else del_qual)
    return conf


def indelqual_arrays(caller, rd, conf):
    """lfq_indelqual_batch on a packed batch (lfq_baq_reads) -> (bi, bd): tag bytes (quality + 33) in the seq_off layout"""
    n = int(rd.n_reads)
    n_bases = int(np.frombuffer((C.c_char * (8 * (n + 1))).from_address(rd.seq_off), np.int64)[-1]) if n else 0
    bi = np.zeros(max(n_bases, 1), np.uint8)
    bd = np.zeros(max(n_bases, 1), np.uint8)
    _lib.check(_lib.load().lfq_indelqual_batch(caller.h, C.byref(rd), C.byref(conf), bi.ctypes.data, bd.ctypes.data),
               "lfq_indelqual_batch")
    return bi[:n_bases], bd[:n_bases]


def indelqual_batch(caller, reads, ref, mode="dindel", ins_qual=0, del_qual=None):
    """reads: list of dicts {pos0, cigar [(op, len)], seq, qual} of mapped reads of one contig (the caller leaves out the
    reads with UNMAP | SECONDARY | QCFAIL | DUP in Dindel mode); ref: the contig (bytes).
    -> per read (BI, BD) as bytes objects: the Z tags without their NUL"""
    rd, keep = pack_reads(reads, ref)
    bi, bd = indelqual_arrays(caller, rd, make_conf(mode, ins_qual, del_qual))
    seq_off = keep[2]
    del keep
    return [(bi[seq_off[i]:seq_off[i + 1]].tobytes(), bd[seq_off[i]:seq_off[i + 1]].tobytes()) for i in range(len(reads))]


def readset_indelqual(rs, mode="dindel", ins_qual=0, del_qual=None):
    """lfq_readset_indelqual: BI / BD of a ReadSet created without them, computed and kept on the device"""
    conf = make_conf(mode, ins_qual, del_qual)
    _lib.check(rs.L.lfq_readset_indelqual(rs.caller.h, rs.h, C.byref(conf)), "lfq_readset_indelqual")


def readset_fetch_indelquals(rs):
    """lfq_readset_fetch_indelquals -> (bi, bd) tag bytes in the seq_off layout"""
    nb = int(rs.seq_off[-1])
    bi = np.zeros(max(nb, 1), np.uint8)
    bd = np.zeros(max(nb, 1), np.uint8)
    _lib.check(rs.L.lfq_readset_fetch_indelquals(rs.caller.h, rs.h, bi.ctypes.data, bd.ctypes.data),
               "lfq_readset_fetch_indelquals")
    return bi[:nb], bd[:nb]


def last_times(caller):
    """device time of the kernels of the caller's last indelqual call, their launches, its reads and bases"""
    t = _lib.IndelqualTimes()
    _lib.check(_lib.load().lfq_last_indelqual_times(caller.h, C.byref(t)), "lfq_last_indelqual_times")
    return {"ms_kernels": float(t.ms_kernels), "n_launches": int(t.n_launches), "n_reads": int(t.n_reads),
            "n_bases": int(t.n_bases)}
