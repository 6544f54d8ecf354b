"""-m gpu: what lfq_readset_create_from_bam and lfq_readset_encode_bam share on the host -- the descriptor refusals of an
lfq_bam_records, the grow-only buffers of a context, the road of records that lie in pinned memory, and the two timers -- against
tests/bam_records.py::expected_arrays and tests/bam_write_model.py::rewrite."""
import ctypes as C
import functools

import numpy as np
import pytest

import bam_records as br
import bam_write_model as wm

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

LFQ_ERR_INVALID = -1
REF = wm.REF
ARRAYS = ("data", "data_off", "pos", "flag", "mapq", "l_qname", "n_cigar", "l_qseq")
UNIFORM_QUALS = (40, 30)


def _from(la, caller, recs):
    return la.ReadSet.from_bam_records(caller, *[recs[k] for k in ARRAYS], recs["ref"])


def _check_decode(rs, recs, E=None):
    E = br.expected_arrays(recs) if E is None else E
    seq, qual, bi, bd, fl = rs.fetch_bases()
    assert np.array_equal(rs.seq_off, E["seq_off"]) and np.array_equal(fl, E["flags"])
    for name, got in (("seq", seq), ("qual", qual), ("bi", bi), ("bd", bd)):
        bad = np.flatnonzero(got != E[name])
        assert bad.size == 0, (name, bad[:8], got[bad[:8]], E[name][bad[:8]])


def _check_encode(rs, recs, what, given=None):
    """the read set made of `recs` (or of `given`, the same records elsewhere in memory) after a uniform indelqual -> its encode
    equals the model's"""
    rs.indelqual("uniform", *UNIFORM_QUALS)
    bi, bd = rs.fetch_indelquals()
    got = rs.encode_bam(recs if given is None else given, None, what)
    want = wm.rewrite(recs, None, what, recs["pos"], wm.record_cigars(recs), None, None, None, None, bi, bd, wm.UNIFORM)
    for k in ("src", "data_off", "pos", "n_cigar", "flag", "mapq", "l_qname", "l_qseq"):
        assert np.array_equal(got[k], want[k]), (k, got[k][:8], want[k][:8])
    bad = np.flatnonzero(got["data"] != want["data"]) if len(got["data"]) == len(want["data"]) else None
    assert bad is not None and bad.size == 0, bad[:8]
    return want


# ---- 1. descriptor refusals: one table for both entries ----------------------------------------------------------------------------
# name -> (what the row does to the arrays of three valid records, the decode's return code, the encode's on a matching read set).
# An array set to None goes in as a null pointer.  The last record has no aux block: it is exactly as long as its fixed part.

def _decreasing(a):
    a["data_off"][2] = a["data_off"][1] - 1


def _negative(a):
    a["l_qseq"][1] = -1


def _short(a):
    a["data_off"][3] -= 1


def _null(k):
    def f(a):
        a[k] = None
    return f


REFUSALS = {"data_off_decreasing": (_decreasing, LFQ_ERR_INVALID, LFQ_ERR_INVALID),
            "l_qseq_negative": (_negative, LFQ_ERR_INVALID, LFQ_ERR_INVALID),
            "record_one_byte_shorter_than_its_fixed_part": (_short, LFQ_ERR_INVALID, LFQ_ERR_INVALID),
            "ref_null": (_null("ref"), LFQ_ERR_INVALID, 0)}
REFUSALS.update({"%s_null" % k: (_null(k), LFQ_ERR_INVALID, LFQ_ERR_INVALID) for k in ARRAYS})


def _c_records(a):
    from lofreq_amd import _lib
    rc = _lib.BamRecords()
    rc.n_reads = 3
    for k in ARRAYS:
        setattr(rc, k, None if a[k] is None else a[k].ctypes.data)
    rc.ref = None if a["ref"] is None else C.cast(C.c_char_p(a["ref"]), C.c_void_p)
    rc.ref_len = len(REF)
    return rc


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_descriptor_refusals(caller, name):
    import lofreq_amd as la
    from lofreq_amd import _lib
    L = _lib.load()
    mutate, decode_rc, encode_rc = REFUSALS[name]
    good = br.encode([br.mk(8, 1), br.mk(21, 3), br.mk(13, 2, tags=None)], ref=REF)
    assert good["data_off"][3] - good["data_off"][2] == good["l_qname"][2] + 4 + 7 + 13
    a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
    mutate(a)
    rs = _from(la, caller, good)
    rc = _c_records(a)
    out = C.c_void_p(0xdead)
    assert L.lfq_readset_create_from_bam(caller.h, C.byref(rc), C.byref(out)) == decode_rc
    assert out.value is None
    enc = C.cast(C.c_void_p(0xdead0), C.POINTER(_lib.BamEncoded))
    assert L.lfq_readset_encode_bam(caller.h, rs.h, C.byref(rc), None, wm.VITERBI, C.byref(enc)) == encode_rc
    assert bool(enc) == (encode_rc == 0)
    rs.close()
    # the next valid call of either kind on the same context
    rs = _from(la, caller, good)
    _check_decode(rs, good)
    assert la.last_bam_decode_times(caller)["n_launches"] == 2
    _check_encode(rs, good, wm.VITERBI | wm.INDELQUAL)
    assert la.last_bam_encode_times(caller)["n_launches"] == 2
    rs.close()


# ---- 2. the buffers of a context grow and are kept -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _batch(n, first_offset=0, seed0=0):
    """n reads of 150 bases with BI and BD -> (records, expected_arrays): 200 of them are 108 KB, beyond the 64 KiB the pinned
    blocks begin with"""
    recs = br.encode([br.mk(150, seed0 + i, pos0=i) for i in range(n)], ref=REF, first_offset=first_offset)
    return recs, br.expected_arrays(recs)


def test_buffers_grow_and_are_kept(caller):
    import lofreq_amd as la
    fresh = la.SnvCaller(0)                                 # a context whose buffers do not exist yet
    try:
        for n, seed0 in ((3, 0), (200, 0), (3, 500)):
            recs, E = _batch(n, 0, seed0)
            assert (n == 200) == (recs["data_off"][-1] > (1 << 16))
            rs = _from(la, fresh, recs)
            _check_decode(rs, recs, E)
            want = _check_encode(rs, recs, wm.INDELQUAL)
            assert (n == 200) == (want["data_off"][-1] > (1 << 16))
            rs.close()
    finally:
        fresh.close()


# ---- 3. records in pinned memory: no staging copy ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("first_offset", [0, 1])
def test_records_in_pinned_memory(caller, first_offset):
    import torch
    import lofreq_amd as la
    recs, E = _batch(200, first_offset)
    t = torch.empty(len(recs["data"]), dtype=torch.uint8, pin_memory=True)
    assert t.is_pinned()
    view = t.numpy()
    view[:] = recs["data"]
    pinned = dict(recs, data=view)
    assert pinned["data"].ctypes.data == t.data_ptr() and recs["data_off"][0] == first_offset
    rs = _from(la, caller, pinned)
    _check_decode(rs, recs, E)
    _check_encode(rs, recs, wm.VITERBI | wm.INDELQUAL, given=pinned)
    rs.close()


# ---- 4. the two timers stay apart -----------------------------------------------------------------------------------------------------------

def test_decode_times_and_encode_times_stay_apart(caller):
    import lofreq_amd as la
    n, m = 5, 3
    recs_m, E = _batch(m)
    set_m = la.ReadSet.from_arrays(caller, dict(E, n=m, ref=REF))         # (not through the decode: its times stay those of n)
    recs_n, _ = _batch(n)
    set_n = _from(la, caller, recs_n)
    before = la.last_bam_decode_times(caller)
    set_m.encode_bam(recs_m, None, wm.VITERBI)
    dec, enc = la.last_bam_decode_times(caller), la.last_bam_encode_times(caller)
    assert dec["n_reads"] == n and enc["n_reads"] == m
    assert dec["n_launches"] == 2 and enc["n_launches"] == 2
    assert dec["n_data_bytes"] == int(recs_n["data_off"][-1]) and dec == before
    assert enc["n_in_bytes"] == int(recs_m["data_off"][-1])
    set_m.close()
    set_n.close()
