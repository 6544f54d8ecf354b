"""Rate of `lofreq uniq` on a resident read set -> profiles/readset_uniq_rate.json

  shape     the chain's region shape: 2 000 000 position-sorted reads of 150 bases over 1 Mb (300x), no BAQ (uniq's mpileup);
            1 000 / 10 000 / 100 000 SNV variants at positions drawn uniformly, AF drawn from a few values.
  roads     (a) lfq_readset_uniq, default mode and --use-det-lim, with the two kernels' device time (lfq_last_sites_times)
            (b) what a caller had before, sparse: per variant lfq_readset_pileup_snv(rs, p, p + 1) + lfq_uniq_binom_batch --
                one search, one scan and one set of launches per variant; 1 000 sites only
            (c) what a caller had before, dense: ONE lfq_readset_pileup_snv over the whole span (the columns of every position;
                the uniq tests on the picked columns would come on top)
  timing    wall time of the calls from the host (C functions through ctypes, results on the host on return), after a warm-up:
            min and median of 7 per road.
  verdicts  a_beats_b: (b)'s min minus (a)'s median at 1 000 sites exceeds (b)'s own min-to-median spread;
            a_over_c[n]: (a)'s median over (c)'s median at each site count (above 1: the dense road is the faster one there).

    python profiles/readset_uniq_rate.py [out.json]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_READS, RL, GLEN, REPS = 2000000, 150, 1000000, 7
SITES = (1000, 10000, 100000)


def make_reads(seed=5):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, GLEN).astype(np.uint8)
    pos = np.sort(rng.integers(0, GLEN - RL, N_READS)).astype(np.int32)
    seq = np.empty(N_READS * RL, np.uint8)
    qual = np.empty(N_READS * RL, np.uint8)
    step = 100000
    for r0 in range(0, N_READS, step):                      # in parts: the index array of all reads at once is gigabytes
        r1 = min(r0 + step, N_READS)
        part = g[pos[r0:r1, None].astype(np.int64) + np.arange(RL, dtype=np.int64)[None, :]].reshape(-1)
        err = rng.random(part.size, dtype=np.float32) < 0.004
        part[err] = (part[err] + rng.integers(1, 4, int(err.sum())).astype(np.uint8)) & 3
        seq[r0 * RL:r1 * RL] = part
        qual[r0 * RL:r1 * RL] = rng.integers(2, 42, part.size, dtype=np.uint8)
    return {"n": N_READS, "ref": np.frombuffer(b"ACGT", np.uint8)[g].tobytes(), "pos": pos,
            "cig_off": np.arange(N_READS + 1, dtype=np.int64), "cig": np.full(N_READS, RL << 4, np.uint32),
            "seq_off": np.arange(N_READS + 1, dtype=np.int64) * RL, "seq": seq, "qual": qual,
            "mapq": rng.choice(np.asarray([60, 60, 60, 30, 255], np.uint8), N_READS), "rev": rng.integers(0, 2, N_READS, dtype=np.uint8)}


def stats(v):
    return {"min_ms": float(min(v)), "median_ms": float(np.median(v)), "all_ms": [round(float(x), 3) for x in sorted(v)]}


def timed(fn, reps=REPS):
    fn()                                                    # warm-up: allocations grow once
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    import lofreq_amd as la
    from lofreq_amd import _lib
    L = _lib.load()
    cl = la.SnvCaller(0)
    R = make_reads()
    rs = la.ReadSet.from_arrays(cl, R)
    rng = np.random.default_rng(6)
    res = {"shape": {"reads": N_READS, "read_len": RL, "span": GLEN, "depth": N_READS * RL // GLEN}, "reps": REPS, "a": {}, "b": {}, "c": {}}
    for n in SITES:
        pos = rng.integers(0, GLEN, n).astype(np.int64)
        ref_l = [R["ref"][p:p + 1] for p in pos]
        alt_l = [b"ACGT"[(b"ACGT".index(r) + 1) % 4:][:1] for r in ref_l]
        af = rng.choice(np.asarray([0.01, 0.05, 0.2], np.float32), n)
        ref_off = np.arange(n + 1, dtype=np.int64)
        ref_b, alt_b = b"".join(ref_l), b"".join(alt_l)
        v, o = _lib.UniqVariants(), _lib.UniqResult()
        v.n, v.pos, v.ref_off, v.alt_off, v.af = n, pos.ctypes.data, ref_off.ctypes.data, ref_off.ctypes.data, af.ctypes.data
        v.ref, v.alt = C.cast(C.c_char_p(ref_b), C.c_void_p), C.cast(C.c_char_p(alt_b), C.c_void_p)
        outs = {"coverage": np.zeros(n, np.int32), "alt_count": np.zeros(n, np.int32), "uq": np.zeros(n, np.int32),
                "pvalue": np.zeros(n, np.float64), "detectable": np.zeros(n, np.uint8)}
        for k, a in outs.items():
            setattr(o, k, a.ctypes.data)
        for mode, det in (("default", 0), ("det_lim", 1)):
            t = timed(lambda: _lib.check(L.lfq_readset_uniq(cl.h, rs.h, C.byref(v), det, 3, C.byref(o)), "lfq_readset_uniq"))
            st = rs.last_sites_times()
            res["a"]["%s_%d" % (mode, n)] = dict(stats(t), count_kernel_ms=st.count_ms, scatter_kernel_ms=st.scatter_ms,
                                                 n_obs=int(st.n_obs), n_launches=int(st.n_launches))
            print("a", mode, n, res["a"]["%s_%d" % (mode, n)], flush=True)
        if n == SITES[0]:
            tr, cp = _lib.Tracks(), np.zeros(1, np.int64)
            uq, alt1 = np.zeros(1, np.int32), np.frombuffer(b"".join(alt_l), np.uint8).copy()

            def sparse_before():
                for i in range(n):
                    p = int(pos[i])
                    _lib.check(L.lfq_readset_pileup_snv(cl.h, rs.h, p, p + 1, 3, C.byref(tr), cp.ctypes.data))
                    if tr.ncols:
                        _lib.check(L.lfq_uniq_binom_batch(cl.h, C.byref(tr), 1, af[i:i + 1].ctypes.data, alt1[i:i + 1].ctypes.data,
                                                          uq.ctypes.data, None))
            res["b"]["default_%d" % n] = stats(timed(sparse_before))
            print("b", n, res["b"]["default_%d" % n], flush=True)

    tr2, cp2 = _lib.Tracks(), np.zeros(GLEN, np.int64)

    def dense_before():
        _lib.check(L.lfq_readset_pileup_snv(cl.h, rs.h, 0, GLEN, 3, C.byref(tr2), cp2.ctypes.data), "lfq_readset_pileup_snv")
        _lib.check(L.lfq_synchronize(cl.h), "lfq_synchronize")
    res["c"]["pileup_snv_span"] = stats(timed(dense_before))
    print("c", res["c"], flush=True)
    a0, b0 = res["a"]["default_%d" % SITES[0]], res["b"]["default_%d" % SITES[0]]
    res["a_beats_b"] = bool(b0["min_ms"] - a0["median_ms"] > b0["median_ms"] - b0["min_ms"])
    res["b_over_a"] = b0["median_ms"] / a0["median_ms"]
    c_med = res["c"]["pileup_snv_span"]["median_ms"]
    res["a_over_c"] = {k: v["median_ms"] / c_med for k, v in res["a"].items()}
    rs.close()
    cl.close()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "readset_uniq_rate.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: res[k] for k in ("a_beats_b", "b_over_a", "a_over_c")}))


if __name__ == "__main__":
    main()
