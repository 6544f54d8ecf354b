"""-m gpu: lfq_viterbi_batch (the viterbi realigner on the device) through the C ABI.

  * position, CIGAR and status of every read of both fixture families (tests/golden/viterbi_*.json) are the reference's 2.1.4
    binary's, with the default -q and with -q 20;
  * a randomised batch of more than 20 000 reads of 36 to 340 bases is the Python model's (tests/viterbi_model.py), read for
    read, in both -q modes;
  * the same batch twice, cut into uneven sub-batches, and in a process whose scratch budget forces many launches gives the
    same arrays;
  * an empty batch and a batch of reads that are left alone launch nothing and return their input;
  * the realigned reads, sorted again, go through the resident read-set chain with --call-indels and give the VCF lines of
    tests/oracle_chain.py on the same reads.
Integers and strings only: no tolerance anywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import viterbi_model as vm
import viterbi_reads as vr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1500)]

HERE = os.path.dirname(os.path.abspath(__file__))
DEF_QUALS = (-1, 20)
RANDOM = dict(seed=9107, n=20480, glen=6000)


def _run(caller, reads, genome, def_qual):
    from lofreq_amd import viterbi as lv
    return lv.viterbi_batch(caller, [vr.lib_read(r) for r in reads], genome.encode(), def_qual)


def _arrays(caller, reads, genome, def_qual):
    from lofreq_amd import viterbi as lv
    rd, keep = lv.pack_reads([vr.lib_read(r) for r in reads], genome.encode())
    out = lv.viterbi_arrays(caller, rd, def_qual)
    del keep
    return out


@pytest.mark.parametrize("name", ["viterbi_small", "viterbi_shapes"])
def test_every_fixture_read_is_the_binarys(caller, name):
    from test_viterbi_model import fixture_reads
    fx, genome, reads = fixture_reads(name)
    assert vr.sha256(vr.sam_text(genome, reads)) == fx["sam_sha256"]
    for dq in DEF_QUALS:
        got = _run(caller, reads, genome, dq)
        want = fx["results"][str(dq)]
        assert len(got) == len(want) == len(reads)
        bad = [(r["name"], dq, (p, vm.cigar_str(c)), tuple(w)) for r, (p, c, s), w in zip(reads, got, want)
               if [p, vm.cigar_str(c)] != w]
        assert not bad, (len(bad), bad[:5])
        for r, (p, c, s) in zip(reads, got):
            kind = s & 7
            expect = {"plain": vm.NO_INDEL, "hclip": vm.SKIPPED_OP, "nop": vm.SKIPPED_OP, "allq2": vm.ALL_Q2}.get(r["shape"],
                                                                                                               vm.REALIGNED)
            assert kind == expect, (r["name"], r["shape"], s)
            changed = (p, c) != (r["pos0"], [tuple(x) for x in r["cigar"]])
            assert bool(s & vm.CHANGED) == changed and (kind == vm.REALIGNED or not changed), (r["name"], s)


def test_randomised_batch_is_the_models_read_for_read(caller):
    from test_viterbi_model import model_results
    R = vr.make(**RANDOM)
    reads, genome = R["reads"], R["genome"]
    assert len(reads) >= 20000 and sum(1 for r in reads if len(r["seq"]) >= 300) >= 500
    want = model_results(genome, reads)
    for dq in DEF_QUALS:
        got = _run(caller, reads, genome, dq)
        bad = [(r["name"], dq, g, w) for r, g, w in zip(reads, ((p, vm.cigar_str(c), s) for p, c, s in got), want[dq]) if g != w]
        assert not bad, (len(bad), bad[:5])
    from lofreq_amd import viterbi as lv
    t = lv.last_times(caller)
    assert t["n_reads"] == len(reads) and t["n_realigned"] == sum(1 for w in want[20] if w[2] & 7 == vm.REALIGNED) > 10000
    assert t["n_launches"] >= 1 and t["ms_kernels"] > 0


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def test_batch_neighbours_and_chunking_do_not_matter(caller):
    R = vr.make(seed=9108, n=6000, glen=4000)
    reads, genome = R["reads"], R["genome"]
    whole = _arrays(caller, reads, genome, -1)
    assert _same(whole, _arrays(caller, reads, genome, -1))
    cuts = [0, 1, 78, 79, 2500, 2500, 5999, 6000]
    pos, status, cig = [], [], []
    for a, b in zip(cuts, cuts[1:]):
        p, s, off, c = _arrays(caller, reads[a:b], genome, -1)
        assert len(p) == len(s) == b - a and off[0] == 0 and off[-1] == len(c)
        pos.append(p), status.append(s), cig.append(c)
    assert np.array_equal(np.concatenate(pos), whole[0]) and np.array_equal(np.concatenate(status), whole[1])
    assert np.array_equal(np.concatenate(cig), whole[3])
    # reversed order: a read's result does not depend on where it stands
    rev = _run(caller, reads[::-1], genome, -1)[::-1]
    fwd = _run(caller, reads, genome, -1)
    assert rev == fwd
    # a fresh process whose scratch budget is 4 MiB cuts the batch into many launches
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "lfq_viterbi_chunks_%d.npz" % os.getpid())
    env = dict(os.environ, LFQ_BAQ_SCRATCH_MB="4")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "9108", "6000", "4000", out], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(out)
    os.remove(out)
    assert int(z["n_launches"]) > 20
    assert _same(whole, (z["pos"], z["status"], z["cigar_off"], z["cigar"]))


def test_nothing_to_realign_launches_nothing(caller):
    from lofreq_amd import viterbi as lv
    R = vr.make(seed=9109, n=600, glen=3000)
    genome = R["genome"]
    assert _run(caller, [], genome, -1) == []
    assert lv.last_times(caller) == {"ms_kernels": 0.0, "n_launches": 0, "n_reads": 0, "n_realigned": 0}
    alone = [r for r in R["reads"] if r["shape"] in ("plain", "hclip", "nop", "allq2")]
    assert len(alone) > 60 and {r["shape"] for r in alone} == {"plain", "hclip", "nop", "allq2"}
    got = _run(caller, alone, genome, -1)
    assert [(p, c) for p, c, _ in got] == [(r["pos0"], [tuple(x) for x in r["cigar"]]) for r in alone]
    assert {s for _, _, s in got} == {vm.NO_INDEL, vm.SKIPPED_OP, vm.ALL_Q2}
    t = lv.last_times(caller)
    assert t["n_launches"] == 0 and t["n_realigned"] == 0 and t["n_reads"] == len(alone) and t["ms_kernels"] == 0.0


def test_bad_arguments_are_refused(caller):
    from lofreq_amd import _lib, viterbi as lv
    R = vr.make(seed=9110, n=60, glen=1500)
    rd, keep = lv.pack_reads([vr.lib_read(r) for r in R["reads"]], R["genome"].encode())
    res = C.POINTER(_lib.ViterbiResult)()
    L = _lib.load()
    assert L.lfq_viterbi_batch(caller.h, C.byref(rd), 94, C.byref(res)) == -1           # -q above the quality range
    assert L.lfq_viterbi_batch(caller.h, None, -1, C.byref(res)) == -1
    keep[5][:] = 120                                                                    # qualities above 93
    assert L.lfq_viterbi_batch(caller.h, C.byref(rd), -1, C.byref(res)) == -1


# ---- realigned reads through the reads -> VCF chain -------------------------------------------------------------------

def _realign_flat(caller, R, def_qual=-1):
    """the flat read arrays of tests/golden_reads.py realigned and sorted again -> (new arrays, status per input read)"""
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
    pos, status, cig_off, cig = lv.viterbi_arrays(caller, rd, def_qual)
    n = int(R["n"])
    order = np.argsort(pos, kind="stable")
    so = np.asarray(R["seq_off"], np.int64)
    base_idx = np.concatenate([np.arange(so[i], so[i + 1]) for i in order]) if n else np.zeros(0, np.int64)
    cig_idx = np.concatenate([np.arange(cig_off[i], cig_off[i + 1]) for i in order]) if n else np.zeros(0, np.int64)
    N = dict(R)
    N["pos"] = pos[order]
    N["cig"] = cig[cig_idx]
    N["cig_off"] = np.concatenate([[0], np.cumsum(np.diff(cig_off)[order])]).astype(np.int64)
    N["seq_off"] = np.concatenate([[0], np.cumsum(np.diff(so)[order])]).astype(np.int64)
    for k in ("seq", "qual", "bi", "bd"):
        if R.get(k) is not None:
            N[k] = np.asarray(R[k])[base_idx]
    for k in ("mapq", "rev", "flags"):
        N[k] = np.asarray(R[k])[:n][order]
    N["lb"] = N["ai"] = N["ad"] = None
    return N, status


def _both_chains(la, caller, oracle, R, ndf=True):
    import golden_util as gu
    import oracle_chain as oc
    from test_gpu_big_golden import device_chain
    kw = dict(flag=la.LFQ_USE_BAQ | la.LFQ_USE_MQ | la.LFQ_USE_IDAQ)
    lines, conf, n_indel_tests = device_chain(la, caller, R, kw, ndf)
    P = dict(R)
    oracle.baq_idaq_reads(P, extended=True, idaq=True, procs=min(16, len(os.sched_getaffinity(0))))
    out = oc.call_region(oracle, P, R["ref"], 0, R["glen"], kw, call_indels=True, no_default_filter=ndf)
    assert conf.num_snv_tests == out["n_snv_tests"] and n_indel_tests == out["n_indel_tests"]
    assert [gu.strip_hqa(l) for l in lines] == [gu.strip_hqa(l) for l in out["lines"]]
    return lines


def test_realigned_reads_go_through_the_indel_calling_chain(caller, oracle):
    import golden_reads as gr
    import lofreq_amd as la
    R = gr.make(seed=612, glen=3000, depth_lo=150, depth_hi=250, min_q=6, snv_every=40, indel_every=120)
    N, status = _realign_flat(caller, R)
    assert int(((status & 7) == vm.REALIGNED).sum()) == R["n_indel_reads"] > 100
    assert bool(np.all(np.diff(N["pos"]) >= 0))
    lines = _both_chains(la, caller, oracle, N)
    assert any("INDEL" in l for l in lines) and any("INDEL" not in l for l in lines)


def _at_repeat_reads():
    """146 reads of 100 bases over an (AT)x12 repeat; 36 of them carry the same 2-base deletion, written at the left end, in
    the middle and at the right end of the repeat (12 each)"""
    rng = np.random.default_rng(77)
    glen, rl, rep0, nrep = 600, 100, 290, 12
    g = rng.integers(0, 4, glen).astype(np.uint8)
    g[rep0 - 1], g[rep0 + 2 * nrep] = 2, 1                  # G (AT)x12 C
    g[rep0:rep0 + 2 * nrep] = np.tile([0, 3], nrep)
    reads = []
    for i in range(146):
        p = 215 + (i * 7) % 60
        if i % 4 == 0 and i < 144:
            at = rep0 + (0, 10, 22)[(i // 4) % 3]           # the deleted pair: first, sixth, last unit
            a = at - p
            seq = np.concatenate([g[p:at], g[at + 2:p + rl + 2]])
            reads.append((p, [(a << 4), (2 << 4) | 2, ((rl - a) << 4)], seq))
        else:
            reads.append((p, [rl << 4], g[p:p + rl].copy()))
    reads.sort(key=lambda r: r[0])
    n = len(reads)
    R = {"n": n, "rl": rl, "glen": glen, "ref": np.frombuffer(b"ACGT", np.uint8)[g].tobytes(),
         "pos": np.asarray([r[0] for r in reads], np.int32),
         "cig_off": np.concatenate([[0], np.cumsum([len(r[1]) for r in reads])]).astype(np.int64),
         "cig": np.asarray([w for r in reads for w in r[1]], np.uint32),
         "seq_off": np.arange(n + 1, dtype=np.int64) * rl, "seq": np.concatenate([r[2] for r in reads]).astype(np.uint8),
         "qual": np.full(n * rl, 35, np.uint8), "bi": np.full(n * rl, 33 + 40, np.uint8), "bd": np.full(n * rl, 33 + 40, np.uint8),
         "ai": None, "ad": None, "lb": None, "sq": None, "flags": np.full(n, 3, np.uint8), "mapq": np.full(n, 60, np.uint8),
         "rev": (np.arange(n) % 2).astype(np.uint8), "n_indel_reads": sum(len(r[1]) == 3 for r in reads)}
    assert R["n_indel_reads"] == 36
    return R


def test_one_deletion_written_at_three_places_of_an_at_repeat(caller, oracle):
    import lofreq_amd as la
    R = _at_repeat_reads()
    before = _both_chains(la, caller, oracle, R)
    N, status = _realign_flat(caller, R)
    assert int(((status & 7) == vm.REALIGNED).sum()) == 36
    after = _both_chains(la, caller, oracle, N)
    n_before, n_after = sum("INDEL" in l for l in before), sum("INDEL" in l for l in after)
    print("indel records before realignment: %d, after: %d" % (n_before, n_after))
    for l in before + ["--"] + after:
        if "INDEL" in l or l == "--":
            print(l)
    assert n_after <= n_before


if __name__ == "__main__":
    # the chunking check's child: realign the seeded batch under this process's scratch budget and save the arrays
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import lofreq_amd as la
    from lofreq_amd import viterbi as lv
    seed, n, glen, path = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    R = vr.make(seed=seed, n=n, glen=glen)
    cl = la.SnvCaller(0)
    rd, keep = lv.pack_reads([vr.lib_read(r) for r in R["reads"]], R["genome"].encode())
    pos, status, cig_off, cig = lv.viterbi_arrays(cl, rd, -1)
    np.savez(path, pos=pos, status=status, cigar_off=cig_off, cigar=cig, n_launches=lv.last_times(cl)["n_launches"])
    cl.close()
