"""-m gpu: lfq_readset_viterbi -- the reads of a resident read set realigned into a NEW read set, through the C ABI.

Two roads from the same host arrays to a realigned read set that is ready for BAQ:
  host road      lfq_viterbi_batch -> stable argsort of the new positions -> repack on the host -> ReadSet (what
                 tests/test_gpu_viterbi.py does)
  resident road  ReadSet(...).viterbi()
Everything compared is an integer or text and is compared for equality: positions, status bytes, CIGAR words, the order, the
tag bytes BAQ / IDAQ write for the permuted bases and qualities, every count of the indel columns, VCF lines."""
import ctypes as C
import functools

import numpy as np
import pytest

import viterbi_model as vm
import viterbi_reads as vr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1500)]

DEF_QUALS = (-1, 20)
OPS = "MIDNSHP=X"
LFQ_ERR_INVALID = -1


# ---- reads as flat arrays (the layout of ReadSet.from_arrays / tests/golden_reads.py) ---------------------------------

def flat(reads, genome):
    """reads of tests/viterbi_reads.py (letters) or dicts with "codes" -> flat arrays; mapq / strand made up per read"""
    n = len(reads)
    codes = [np.asarray(r["codes"], np.uint8) if "codes" in r else vr.lib_read(r)["seq"] for r in reads]
    cig = [(l << 4) | OPS.index(o) for r in reads for o, l in r["cigar"]]
    return {"n": n, "glen": len(genome), "ref": genome.encode(),
            "pos": np.asarray([r["pos0"] for r in reads], np.int32).reshape(n),
            "cig_off": np.concatenate([[0], np.cumsum([len(r["cigar"]) for r in reads])]).astype(np.int64),
            "cig": np.asarray(cig if cig else [0], np.uint32),
            "seq_off": np.concatenate([[0], np.cumsum([len(c) for c in codes])]).astype(np.int64),
            "seq": np.concatenate(codes + [np.zeros(1, np.uint8)]).astype(np.uint8),
            "qual": np.concatenate([np.asarray(r["qual"], np.uint8) for r in reads] + [np.zeros(1, np.uint8)]).astype(np.uint8),
            "mapq": (20 + (np.arange(max(n, 1)) * 7) % 41).astype(np.uint8), "rev": (np.arange(max(n, 1)) % 2).astype(np.uint8),
            "flags": np.zeros(max(n, 1), np.uint8), "bi": None, "bd": None, "lb": None}


def host_result(caller, R, def_qual):
    from lofreq_amd import _lib, viterbi as lv
    keep = {k: np.ascontiguousarray(R[k], dt) for k, dt in (("pos", np.int32), ("cig_off", np.int64), ("cig", np.uint32),
                                                            ("seq_off", np.int64), ("seq", np.uint8), ("qual", np.uint8))}
    ref = bytes(R["ref"])
    rd = _lib.BaqReads()
    rd.n_reads = int(R["n"])
    rd.pos, rd.cigar_off, rd.cigar = keep["pos"].ctypes.data, keep["cig_off"].ctypes.data, keep["cig"].ctypes.data
    rd.seq_off, rd.seq, rd.qual = keep["seq_off"].ctypes.data, keep["seq"].ctypes.data, keep["qual"].ctypes.data
    rd.ref = C.cast(C.c_char_p(ref), C.c_void_p)
    rd.ref_len = len(ref)
    return lv.viterbi_arrays(caller, rd, def_qual)


def host_road(caller, R, def_qual=-1):
    """-> (the realigned, re-sorted flat arrays, lfq_viterbi_batch's result, the order)"""
    res = host_result(caller, R, def_qual)
    pos, status, cig_off, cig = res
    n = int(R["n"])
    order = np.argsort(pos, kind="stable")
    so = np.asarray(R["seq_off"], np.int64)
    base_idx = np.concatenate([np.arange(so[i], so[i + 1]) for i in order] + [np.zeros(0, np.int64)]).astype(np.int64)
    cig_idx = np.concatenate([np.arange(cig_off[i], cig_off[i + 1]) for i in order] + [np.zeros(0, np.int64)]).astype(np.int64)
    N = dict(R)
    N["pos"] = pos[order]
    N["cig"] = cig[cig_idx] if len(cig_idx) else np.zeros(1, np.uint32)
    N["cig_off"] = np.concatenate([[0], np.cumsum(np.diff(cig_off)[order])]).astype(np.int64)
    N["seq_off"] = np.concatenate([[0], np.cumsum(np.diff(so)[order])]).astype(np.int64)
    for k in ("seq", "qual", "bi", "bd"):
        if R.get(k) is not None:
            N[k] = np.concatenate([np.asarray(R[k])[base_idx], np.zeros(1, np.uint8)])
    for k in ("mapq", "rev", "flags"):
        N[k] = np.concatenate([np.asarray(R[k])[:n][order], np.zeros(1, np.uint8)])
    return N, res, order


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def tags_of(rs):
    rs.baq(extended=True, idaq=True)
    lb, ai, ad, fl = rs.fetch_tags(idaq=True)
    nb = int(rs.seq_off[-1])
    return lb[:nb], ai[:nb], ad[:nb], fl[: rs.n]


def both_roads(la, caller, R, def_qual=-1, tags=True):
    """run both roads, hold every integer of the resident one against the host one; -> (new ReadSet, result, order, N)"""
    N, want, want_order = host_road(caller, R, def_qual)
    rs = la.ReadSet.from_arrays(caller, R)
    new, got, order = rs.viterbi(def_qual)
    assert same(got, want), [k for k, (x, y) in enumerate(zip(got, want)) if not np.array_equal(x, y)]
    assert order.dtype == np.int64 and np.array_equal(order, want_order)
    assert np.array_equal(new.seq_off, N["seq_off"])
    rs.close()                                  # the new set does not need the old one
    if tags:
        ref_set = la.ReadSet.from_arrays(caller, N)
        t_new, t_ref = tags_of(new), tags_of(ref_set)
        ref_set.close()
        assert same(t_new, t_ref), [k for k, (x, y) in enumerate(zip(t_new, t_ref)) if not np.array_equal(x, y)]
    return new, got, order, N


# ---- 1. result = lfq_viterbi_batch's = the binary's -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["viterbi_small", "viterbi_shapes"])
def test_result_is_the_batch_calls_and_the_binarys(caller, name):
    import lofreq_amd as la
    from test_viterbi_model import fixture_reads
    fx, genome, reads = fixture_reads(name)
    assert vr.sha256(vr.sam_text(genome, reads)) == fx["sam_sha256"]
    R = flat(reads, genome)
    for dq in DEF_QUALS:
        new, (pos, status, cig_off, cig), order, _ = both_roads(la, caller, R, dq)
        new.close()
        want = fx["results"][str(dq)]
        got = [[int(pos[i]), "".join("%d%s" % (int(w) >> 4, OPS[int(w) & 15]) for w in cig[cig_off[i]:cig_off[i + 1]])]
               for i in range(len(reads))]
        bad = [(r["name"], dq, g, w) for r, g, w in zip(reads, got, want) if g != w]
        assert not bad, (len(bad), bad[:5])


# ---- 2. the new set is the host road's set ----------------------------------------------------------------------------

def _cols_equal(a, b):
    from lofreq_amd.indel import _I32
    assert a.ncols == b.ncols and np.array_equal(a.ref_base, b.ref_base) and np.array_equal(a.cons_indel, b.cons_indel)
    for name in _I32:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    for sd in range(2):
        assert a.keys[sd] == b.keys[sd]
        for k in a.sides[sd]:
            assert np.array_equal(a.sides[sd][k], b.sides[sd][k]), (sd, k)


def test_uploaded_bi_bd_travel_with_their_reads(caller):
    import lofreq_amd as la
    G = vr.make(seed=9301, n=400, glen=2500)
    reads = [r for r in G["reads"] if r["shape"] not in ("hclip", "nop")]
    rng = np.random.default_rng(5)
    rng.shuffle(reads)
    R = flat(reads, G["genome"])
    nb = int(R["seq_off"][-1])
    rid = np.repeat(np.arange(R["n"]), np.diff(R["seq_off"]))
    within = np.arange(nb) - R["seq_off"][rid]
    R["bi"] = np.concatenate([33 + 20 + (rid * 7 + within) % 30, [33]]).astype(np.uint8)       # a pattern of its own per read
    R["bd"] = np.concatenate([33 + 20 + (rid * 11 + 3 * within) % 30, [33]]).astype(np.uint8)
    R["flags"] = np.full(R["n"], 3, np.uint8)
    R["flags"][::9] = 1
    R["flags"][4::13] = 0
    new, _, order, N = both_roads(la, caller, R, -1, tags=False)
    assert not np.array_equal(order, np.arange(R["n"]))
    ref_set = la.ReadSet.from_arrays(caller, N)
    cols_new, pos_new = new.pileup_indels(0, R["glen"], min_plp_idq=25)
    cols_ref, pos_ref = ref_set.pileup_indels(0, R["glen"], min_plp_idq=25)
    assert np.array_equal(pos_new, pos_ref) and cols_new.ncols > 100
    assert sum(len(k) for k in cols_new.keys) > 20
    _cols_equal(cols_new, cols_ref)
    new.close()
    ref_set.close()


# ---- 3. the chain: indelqual -> pileups -> --call-indels ---------------------------------------------------------------

def chain_lines(la, caller, rs, glen, kw, ndf, chrom="chr1"):
    """tests/test_gpu_big_golden.py::device_chain on a read set that exists, with `lofreq indelqual --dindel` as a step"""
    rs.baq(extended=True, idaq=True)
    rs.indelqual("dindel")
    conf = la.VarcallConf(**kw)
    lines = []
    cols, col_pos = rs.pileup_indels(0, glen)
    irecs, n_indel_tests = la.call_indels(caller, cols, conf)
    ikeep = la.filter_indel_records(irecs, la.snvqual_thresh(conf.sig, conf.bonf_indel), apply_defaults=not ndf)
    for r, k in zip(irecs, ikeep):
        if k:
            p0 = int(col_pos[int(r["col"])])
            lines.append((p0, 0, la.format_indel_record(chrom, p0, cols, r, "PASS").rstrip("\n")))
    dt = rs.pileup_snv(0, glen)
    la.skip_snv_columns(caller, cols.cons_indel)
    recs, _, _ = caller.call_snvs(dt, conf)
    keep = la.filter_records(recs, la.snvqual_thresh(conf.sig, conf.bonf_subst), apply_defaults=not ndf)
    for r, k in zip(recs, keep):
        if k:
            p0 = int(dt.col_pos[int(r["col"])])
            lines.append((p0, 1, la.format_vcf(np.array([r]), chrom, pos0=np.array([p0]), filter_str="PASS").rstrip("\n")))
    return [l[2] for l in sorted(lines, key=lambda t: (t[0], t[1]))], (conf.num_snv_tests, n_indel_tests)


def _bare(R):
    return dict(R, bi=None, bd=None, lb=None, flags=np.zeros(max(int(R["n"]), 1), np.uint8))


def _chain_on_both_roads(la, caller, R):
    kw = dict(flag=la.LFQ_USE_BAQ | la.LFQ_USE_MQ | la.LFQ_USE_IDAQ)
    R = _bare(R)
    N, _, _ = host_road(caller, R)
    host_set = la.ReadSet.from_arrays(caller, N)
    want = chain_lines(la, caller, host_set, R["glen"], kw, True)
    host_set.close()
    rs = la.ReadSet.from_arrays(caller, R)
    new, result, order = rs.viterbi()
    got = chain_lines(la, caller, new, R["glen"], kw, True)
    new.close()
    rs.close()
    assert got == want
    return got[0], result


def test_chain_after_the_resident_realignment_writes_the_host_roads_vcf(caller):
    import golden_reads as gr
    import lofreq_amd as la
    R = gr.make(seed=612, glen=3000, depth_lo=150, depth_hi=250, min_q=6, snv_every=40, indel_every=120)
    lines, (pos, status, _, _) = _chain_on_both_roads(la, caller, R)
    assert int(((status & 7) == vm.REALIGNED).sum()) == R["n_indel_reads"] > 100
    assert any("INDEL" in l for l in lines) and any("INDEL" not in l for l in lines)


def test_at_repeat_deletion_written_at_three_places_is_one_record(caller):
    import lofreq_amd as la
    from test_gpu_viterbi import _at_repeat_reads
    R = _at_repeat_reads()
    lines, (pos, status, _, _) = _chain_on_both_roads(la, caller, R)
    assert int(((status & 7) == vm.REALIGNED).sum()) == 36
    indels = [l for l in lines if "INDEL" in l]
    print("\n".join(indels))
    assert len(indels) == 1


# ---- 4. small shapes at which the new kernels can go wrong -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _genome():
    rng = np.random.default_rng(4242)
    g = list(rng.choice(list("ACGT"), 1200))
    g[300:324] = "AT" * 12
    g[500:512] = "A" * 12
    g[700:730] = "CAG" * 10
    g[333] = "N"
    g[820:860] = [c.lower() for c in g[820:860]]
    return "".join(g)


def mk(pos0, cigar, qual=None, codes=None, seed=0):
    """a read that follows the contig along its CIGAR (inserted and clipped bases are random)"""
    G = _genome().upper()
    rng = np.random.default_rng(1000 + seed + pos0)
    cigar = [(o, l) for o, l in cigar if l > 0 or o not in "M"]
    seq, x = [], pos0
    for o, l in cigar:
        if o in "M=X":
            seq.extend(vr._CODE[c] for c in G[x:x + l])
            x += l
        elif o in "IS":
            seq.extend(int(v) for v in rng.integers(0, 4, l))
        elif o in "DN":
            x += l
    if codes is not None:
        assert len(codes) == len(seq)
        seq = list(codes)
    if qual is None:
        qual = [int(v) for v in rng.integers(8, 42, len(seq))]
    assert len(qual) == len(seq)
    return {"pos0": pos0, "cigar": cigar, "codes": seq, "qual": qual}


def _del_read(pos0, length, at=None, seed=0, dlen=2):
    at = max(length // 2, 1) if at is None else at
    return mk(pos0, [("M", at), ("D", dlen), ("M", length - at)], seed=seed)


def _shifted(pos0, length, d, seed=0):
    """a read of `length` matches at pos0, reported d bases to the right with its first d bases as an insertion"""
    true = mk(pos0, [("M", length)], seed=seed)
    return {"pos0": pos0 + d, "cigar": [("I", d), ("M", length - d)], "codes": true["codes"], "qual": true["qual"]}


def _cases():
    glen = len(_genome())
    q6 = lambda vals: [2] * (6 - len(vals)) + list(vals)
    iupac = list(range(5, 16)) + [0, 1, 2, 3] * 8
    cases = {
        "n0": [],
        "one read": [_del_read(100, 50)],
        "query lengths at the strip boundaries": [_del_read(200 + 5 * k, L, seed=k) for k, L in enumerate((1, 63, 64, 65, 128, 129))],
        "soft clips at both ends": [mk(150, [("S", 5), ("M", 30), ("D", 3), ("M", 40), ("S", 7)]),
                                    mk(160, [("S", 1), ("M", 20), ("I", 2), ("M", 30), ("S", 1)])],
        "an I directly after the leading S": [mk(295, [("S", 4), ("I", 2), ("M", 60)]), mk(296, [("M", 50)])],
        "H clip and all-Q2 between realigned reads": [
            _del_read(280, 70, seed=1), mk(282, [("H", 5), ("M", 30), ("D", 2), ("M", 30)]), _del_read(284, 64, seed=2),
            mk(286, [("M", 30), ("I", 2), ("M", 30)], qual=[2] * 62), _del_read(288, 65, seed=3)],
        "window clipped at 0": [_del_read(0, 40), _del_read(3, 45, seed=1), _shifted(6, 50, 3), _del_read(9, 30, seed=2)],
        "read ending near the contig end": [_del_read(glen - 62, 60), _del_read(glen - 75, 66, seed=1), mk(glen - 40, [("M", 40)]),
                                            mk(glen - 52, [("M", 30), ("I", 2), ("M", 20)])],
        "median of 1, 2, 3, 4 qualities": [mk(400 + 2 * k, [("M", 3), ("D", 1), ("M", 3)], qual=q6(v))
                                           for k, v in enumerate(([10], [10, 31], [10, 31, 20], [10, 31, 20, 41], [41, 40],
                                                                  [0, 93], [93], [3, 4, 4]))],
        "base codes 5..15 and an N in the reference": [
            mk(315, [("M", 25), ("D", 2), ("M", 18)], codes=iupac, seed=1), mk(320, [("M", 20), ("I", 3), ("M", 20)], codes=iupac),
            mk(325, [("M", 43)], codes=iupac)],
        "realignment swaps two reads": [mk(601, [("M", 50)]), _shifted(600, 60, 3)],
        "three reads with equal new pos, unsorted input": [_shifted(650, 40, 2), mk(650, [("M", 33)]), mk(650, [("M", 51)])],
        "seq_off 1, 15, 16, 17 modulo 16 and a zero-length read": [
            mk(700, [("M", 1)]), _del_read(701, 14, seed=1), mk(702, [("M", 1)]), mk(703, [("M", 1)], seed=3),
            {"pos0": 704, "cigar": [], "codes": [], "qual": []}, _shifted(690, 40, 3), mk(705, [("M", 23)]), _del_read(706, 16, seed=5)],
        "4097 bases": [(_del_read(40 + 7 * k, 150, seed=k) if k % 4 == 0 else _shifted(40 + 7 * k, 150, 1 + k % 4, seed=k)
                        if k % 4 == 1 else mk(40 + 7 * k, [("M", 150)], seed=k)) for k in range(27)] + [mk(600, [("M", 47)])],
    }
    assert sum(len(r["codes"]) for r in cases["4097 bases"]) == 4097
    return cases


@pytest.mark.parametrize("name", sorted(_cases()))
def test_small_shapes_equal_the_host_road(caller, name):
    import lofreq_amd as la
    from lofreq_amd import viterbi as lv
    reads = _cases()[name]
    R = flat(reads, _genome())
    if name.startswith("seq_off"):
        assert [int(v) % 16 for v in R["seq_off"][1:5]] == [1, 15, 0, 1] and 0 in np.diff(R["seq_off"])
    for dq in ((-1,) if name.startswith("median") else DEF_QUALS):
        new, (pos, status, cig_off, cig), order, N = both_roads(la, caller, R, dq)
        t = lv.last_times(caller)
        assert t["n_reads"] == len(reads) and t["n_realigned"] == int(((status & 7) == vm.REALIGNED).sum())
        assert t["n_launches"] == (1 if t["n_realigned"] else 0)
        if name.startswith("realignment swaps"):
            assert list(order) == [1, 0]
        if name.startswith("three reads"):
            assert list(order) == [0, 1, 2] and len(set(int(p) for p in pos)) == 1
        if name.startswith("H clip"):
            assert [int(s) & 7 for s in status] == [vm.REALIGNED, vm.SKIPPED_OP, vm.REALIGNED, vm.ALL_Q2, vm.REALIGNED]
        if name.startswith("median"):
            # q2def decides nothing the model cannot say: hold the reads against tests/viterbi_model.py as well
            for i, r in enumerate(reads):
                p, c, s = vm.realign(dict(r, seq=np.asarray(r["codes"], np.uint8), cigar=[tuple(x) for x in r["cigar"]]),
                                     _genome(), -1)
                assert (int(pos[i]), int(status[i])) == (p, s)
        new.close()


def test_no_read_with_an_indel_launches_nothing(caller):
    import lofreq_amd as la
    from lofreq_amd import viterbi as lv
    reads = [mk(50 + 3 * k, [("S", k % 3), ("M", 30 + k)], seed=k) for k in range(9)]
    R = flat(reads, _genome())
    new, (pos, status, cig_off, cig), order, N = both_roads(la, caller, R)
    assert lv.last_times(caller) == {"ms_kernels": 0.0, "n_launches": 0, "n_reads": 9, "n_realigned": 0}
    assert np.array_equal(order, np.arange(9)) and not status.any() and np.array_equal(pos, R["pos"])
    new.close()
    # unsorted input without an indel: sorted all the same
    R2 = flat(reads[::-1], _genome())
    new, _, order, _ = both_roads(la, caller, R2)
    assert np.array_equal(order, np.arange(9)[::-1])
    new.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------

def _raw_viterbi(caller, rs_handle, def_qual, want_out=True):
    from lofreq_amd import _lib
    h, res, order = C.c_void_p(), C.POINTER(_lib.ViterbiResult)(), C.c_void_p()
    rc = caller.L.lfq_readset_viterbi(caller.h, rs_handle, def_qual, C.byref(h) if want_out else None, C.byref(res),
                                      C.byref(order))
    return rc, h


def test_refusals_leave_the_context_usable(caller):
    import lofreq_amd as la
    G = vr.make(seed=9302, n=80, glen=1500)
    reads = [r for r in G["reads"] if r["shape"] not in ("hclip", "nop")]
    R = flat(reads, G["genome"])
    nb = int(R["seq_off"][-1])
    L = caller.L

    def good():
        new, _, _, _ = both_roads(la, caller, R, tags=False)
        new.close()

    def refused(rs, dq=-1, want_out=True):
        rc, h = _raw_viterbi(caller, rs.h, dq, want_out)
        assert rc == LFQ_ERR_INVALID and not h.value
        good()

    # created with lb
    rs = la.ReadSet.from_arrays(caller, dict(R, lb=np.full(nb + 1, 40, np.uint8)))
    refused(rs)
    rs.close()
    # created with reads->sq: through the struct, the Python class has no such argument
    from lofreq_amd import _lib
    base = la.ReadSet.from_arrays(caller, R)
    keep = base._keep
    rd = _lib.PileupReads()
    rd.n_reads = R["n"]
    rd.pos, rd.cigar_off, rd.cigar = keep["pos"].ctypes.data, keep["cig_off"].ctypes.data, keep["cig"].ctypes.data
    rd.seq_off, rd.seq, rd.qual = keep["seq_off"].ctypes.data, keep["seq"].ctypes.data, keep["qual"].ctypes.data
    rd.mapq, rd.reverse = keep["mapq"].ctypes.data, keep["rev"].ctypes.data
    rd.ref = C.cast(C.c_char_p(keep["ref"]), C.c_void_p)
    rd.ref_len = len(keep["ref"])
    sq = np.full(R["n"], 30, np.uint8)
    rd.sq = sq.ctypes.data
    for with_ai in (False, True):
        tags = _lib.PileupIndelTags()
        if with_ai:
            rd.sq = None
            ai = np.full(nb + 1, 60, np.uint8)
            tags.ai = ai.ctypes.data
        h = C.c_void_p()
        assert L.lfq_readset_create(caller.h, C.byref(rd), C.byref(tags), C.byref(h)) == 0
        rc, out = _raw_viterbi(caller, h, -1)
        L.lfq_readset_destroy(h)
        assert rc == LFQ_ERR_INVALID and not out.value
        good()
    # def_qual above the quality range, out = NULL, and after BAQ
    refused(base, dq=94)
    refused(base, want_out=False)
    base.baq(extended=True, idaq=False)
    refused(base)
    base.close()
    rs = la.ReadSet.from_arrays(caller, R)
    rs.indelqual("uniform", 40)
    refused(rs)
    rs.close()
    rs = la.ReadSet.from_arrays(caller, R)
    rs.source_qual()
    refused(rs)
    rs.close()
    # a quality of 94 in a read that is realigned (and none in a read that is left alone: accepted)
    status = host_result(caller, R, -1)[1] & 7
    r_re, r_alone = int(np.flatnonzero(status == vm.REALIGNED)[0]), int(np.flatnonzero(status == vm.NO_INDEL)[0])
    Q = dict(R, qual=R["qual"].copy())
    Q["qual"][R["seq_off"][r_alone]] = 94
    new, _, _, _ = both_roads(la, caller, Q, tags=False)
    new.close()
    Q["qual"][R["seq_off"][r_re] + (reads[r_re]["cigar"][0][1] if reads[r_re]["cigar"][0][0] == "S" else 0)] = 94
    rs = la.ReadSet.from_arrays(caller, Q)
    refused(rs)
    rs.close()


# ---- 6. the input set is untouched -------------------------------------------------------------------------------------

def test_input_read_set_is_untouched_and_either_destroy_order_works(caller):
    import golden_reads as gr
    import lofreq_amd as la
    R = _bare(gr.make(seed=613, glen=1500, depth_lo=60, depth_hi=90, min_q=6, snv_every=40, indel_every=120))
    kw = dict(flag=la.LFQ_USE_BAQ | la.LFQ_USE_MQ | la.LFQ_USE_IDAQ)
    fresh = la.ReadSet.from_arrays(caller, R)
    want = chain_lines(la, caller, fresh, R["glen"], kw, True)
    fresh.close()
    assert any("INDEL" in l for l in want[0])
    N, _, _ = host_road(caller, R)
    host_set = la.ReadSet.from_arrays(caller, N)
    want_new = chain_lines(la, caller, host_set, R["glen"], kw, True)
    host_set.close()
    for first in ("input", "output"):
        rs = la.ReadSet.from_arrays(caller, R)
        new, result, order = rs.viterbi()
        assert (result[1] & vm.CHANGED).any()
        if first == "input":
            assert chain_lines(la, caller, rs, R["glen"], kw, True) == want
            rs.close()
            assert chain_lines(la, caller, new, R["glen"], kw, True) == want_new
            new.close()
        else:
            assert chain_lines(la, caller, new, R["glen"], kw, True) == want_new
            new.close()
            assert chain_lines(la, caller, rs, R["glen"], kw, True) == want
            rs.close()


# ---- 7. randomised ------------------------------------------------------------------------------------------------------

def test_randomised_batch_is_the_models_and_the_host_roads(caller):
    import lofreq_amd as la
    from test_viterbi_model import model_results
    G = vr.make(seed=9107, n=20000, glen=6000)
    reads, genome = G["reads"], G["genome"]
    R = flat(reads, genome)
    want = model_results(genome, reads, (-1,))[-1]
    new, (pos, status, cig_off, cig), order, _ = both_roads(la, caller, R, -1)
    new.close()
    words = vm.cigar_str
    got = [(int(pos[i]), words([(OPS[int(w) & 15], int(w) >> 4) for w in cig[cig_off[i]:cig_off[i + 1]]]), int(status[i]))
           for i in range(len(reads))]
    bad = [(r["name"], g, w) for r, g, w in zip(reads, got, want) if g != w]
    assert not bad, (len(bad), bad[:5])
    assert int(((status & 7) == vm.REALIGNED).sum()) > 10000


# ---- 8. the read-level binding ---------------------------------------------------------------------------------------------

def _run_binding(caller, lib, region_reads, ref, regions, conf, viterbi, late=False):
    """tests/test_gpu_chain.py::_run_regions with lfq_region_set_viterbi; region_reads[k] = the reads handed in for region k"""
    from test_gpu_chain import _RegionOpts, _bam_fields
    P = C.CDLL(lib)
    lines = []
    EMIT = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)
    cb = EMIT(lambda user, s: lines.append(s.decode().rstrip("\n")))
    o = _RegionOpts()
    P.lfq_region_opts_init(C.byref(o))
    o.use_idaq, o.call_indels = 1, 1
    h = C.c_void_p()
    P.lfq_region_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, EMIT, C.c_void_p]
    assert P.lfq_region_open(C.byref(h), caller.h, C.byref(conf.c), C.byref(o), cb, None) == 0
    P.lfq_region_set_viterbi.argtypes = [C.c_void_p, C.c_int, C.c_int]
    if viterbi is not None and not late:
        assert P.lfq_region_set_viterbi(h, 1, 94) == LFQ_ERR_INVALID
        assert P.lfq_region_set_viterbi(h, 1, viterbi) == 0
    P.lfq_region_begin.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int64]
    P.lfq_region_add_read.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_char_p, C.c_char_p]
    P.lfq_region_end.argtypes = [C.c_void_p]
    P.lfq_region_close.argtypes = [C.c_void_p, C.c_void_p]
    for (beg, end), reads in zip(regions, region_reads):
        assert P.lfq_region_begin(h, b"chr1", ref, len(ref), beg, end) == 0
        if late:
            assert P.lfq_region_set_viterbi(h, 1, -1) == LFQ_ERR_INVALID
        for r in reads:
            seq4, cig, bi, bd = _bam_fields(r)
            q = np.asarray(r["qual"], np.uint8)
            assert P.lfq_region_add_read(h, r["pos0"], 16 if r["reverse"] else 0, r["mapq"], len(cig), cig.ctypes.data, len(q),
                                         seq4.ctypes.data, q.ctypes.data, bi, bd) == 1
        assert P.lfq_region_end(h) == 0
    wo = C.c_int64(-1)
    assert P.lfq_region_close(h, C.byref(wo)) == 0
    return lines


def test_region_binding_with_the_option_equals_the_host_roads_reads(caller, tmp_path):
    import golden_util as gu
    import lofreq_amd as la
    from lofreq_amd import viterbi as lv
    from test_gpu_chain import _build_region_lib
    lib = _build_region_lib(tmp_path)
    fx, reads = gu.load_plpindel(gu.plpindel_fixtures()[-1], with_alnqual_tags=False)
    ref = fx["genome"].encode()
    kw, _ = gu.conf_kwargs(fx["call_args"])
    n = len(ref)

    def overlapping(beg, end):
        return [r for r in reads if not (r["pos0"] >= end or r["pos0"] + sum(l for op, l in r["cigar"] if op in "MDN=X") <= beg)]

    def realigned(rr):
        """the host road on the reads of one region: lfq_viterbi_batch, then the stable sort by new position"""
        out = lv.viterbi_batch(caller, [dict(pos0=r["pos0"], cigar=[tuple(c) for c in r["cigar"]], seq=np.asarray(r["seq"], np.uint8),
                                             qual=np.asarray(r["qual"], np.uint8)) for r in rr], ref, -1)
        new = [dict(r, pos0=p, cigar=c) for r, (p, c, s) in zip(rr, out)]
        return [new[i] for i in np.argsort([r["pos0"] for r in new], kind="stable")], sum((s & 7) == vm.REALIGNED for _, _, s in out)

    for regions in ([(0, n)], [(0, n // 3), (n // 3, n // 3 + 37), (n // 3 + 37, n)]):
        as_given = [overlapping(b, e) for b, e in regions]
        on_host = [realigned(rr) for rr in as_given]
        assert sum(k for _, k in on_host) > 20
        c_on, c_host, c_off, c_late = (la.VarcallConf(**kw) for _ in range(4))
        on = _run_binding(caller, lib, as_given, ref, regions, c_on, -1)
        host = _run_binding(caller, lib, [rr for rr, _ in on_host], ref, regions, c_host, None)
        assert on == host and any("INDEL" in l for l in on)
        assert (c_on.num_snv_tests, c_on.num_indel_tests, c_on.bonf_indel) == (c_host.num_snv_tests, c_host.num_indel_tests, c_host.bonf_indel)
        # default off, and refused once a region has begun: the binding as it was, reads as given
        off = _run_binding(caller, lib, as_given, ref, regions, c_off, None)
        late = _run_binding(caller, lib, as_given, ref, regions, c_late, -1, late=True)
        assert off == late
        from test_gpu_chain import _run_regions
        plain, _, _ = _run_regions(caller, lib, reads, ref, regions, la.VarcallConf(**kw))
        assert off == plain
