"""`lofreq call -l` on the read-level road: the targets on the context (lfq_set_bed) against the road the caller's own BED took
 -> profiles/bed_rate.json

  shape     one bin of bench.py's C5 (make_tile): 2 Mb, ragged targets of 150 .. 3500 bases with gaps of 200 .. 1900 (about 45 % of
            the bin), 200x of all-M reads of 150 bases where they touch a target, SNVs planted every 997th position -- and half as
            many reads again that touch no target, which a caller without a BED of its own hands over too
  roads     (a)  the targets on the context: every read goes up; the read kernel drops the off-target ones in front of BAQ, the
                 column kernel takes the flanks out between the count pass and the column compaction
            (b)  what the project ran before, the caller filtering: the reads its own BED keeps go up (the host's filter is timed
                 apart), the whole bin is piled up, col_pos comes back, numpy builds the off-target byte mask, it goes down through
                 lfq_pileup_skip_snv_columns
            (b0) the same without the caller's read filter: every read through BAQ and both pileup passes
            each from lfq_readset_create to the records on the host: create, BAQ, pileup_snv, (mask,) the SNV calls, records d2h
  timing    wall time from the host, 5 passes after a warm-up, the roads alternating within a pass; median and range.  BAQ kernel
            time and the reads launched: lfq_last_baq_times (device events).  Columns and observations: what the count kernel is
            handed (ncols, col_off[ncols]).  The two new kernels have no event pair of their own: their time is not measured here.

    python profiles/bed_rate.py [out.json]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TILE, DEPTH, RL, PASSES = 2_000_000, 200, 150, 5


def make_bin(seed=11):
    """bench.py::make_tile's C5 bin, plus the off-target reads -> (R with every read, the byte mask of the targets, BED text)"""
    rng = np.random.default_rng(seed + 1)
    target = np.zeros(TILE, np.uint8)
    iv = []
    x = 300
    while x < TILE - 4000:
        l = int(rng.choice([150, 300, 600, 1200, 2000, 3500], p=[0.2, 0.25, 0.2, 0.15, 0.12, 0.08]))
        target[x:x + l] = 1
        iv.append((x, x + l))
        x += l + int(rng.integers(200, 1900))
    cs = np.concatenate([[0], np.cumsum(target, dtype=np.int64)])
    pos = np.sort(rng.integers(0, TILE - RL - 20, int(TILE * DEPTH / RL))).astype(np.int32)
    on = (cs[pos + RL] - cs[pos]) > 0
    n_on = int(on.sum())
    off_idx = np.nonzero(~on)[0]
    off_idx = np.sort(rng.choice(off_idx, min(len(off_idx), n_on // 2), replace=False))
    take = np.zeros(len(pos), bool)
    take[on] = True
    take[off_idx] = True
    pos = np.ascontiguousarray(pos[take])
    n = len(pos)
    genome = rng.integers(0, 4, TILE).astype(np.uint8)
    seq = genome[pos[:, None] + np.arange(RL, dtype=np.int32)[None, :]]
    mism = rng.random(seq.shape, dtype=np.float32) < 0.003
    seq[mism] = (seq[mism] + 1) % 4
    for k, p in enumerate(range(500, TILE - RL - 20, 997)):
        af = (0.005, 0.01, 0.05, 0.5)[k % 4]
        lo, hi = np.searchsorted(pos, p - RL + 1), np.searchsorted(pos, p, side="right")
        idx = np.arange(lo, hi)
        idx = idx[rng.random(len(idx)) < af]
        seq[idx, p - pos[idx]] = (seq[idx, p - pos[idx]] + 1 + k % 3) % 4
    R = {"n": n, "ref": np.frombuffer(b"ACGT", np.uint8)[genome].tobytes(), "pos": pos, "cig_off": np.arange(n + 1, dtype=np.int64),
         "cig": np.full(n, RL << 4, np.uint32), "seq_off": np.arange(n + 1, dtype=np.int64) * RL, "seq": np.ascontiguousarray(seq.reshape(-1)),
         "qual": rng.integers(28, 42, n * RL, dtype=np.uint8), "mapq": np.full(n, 60, np.uint8), "rev": (rng.random(n) < 0.5).astype(np.uint8)}
    return R, target, "".join("synth\t%d\t%d\n" % t for t in iv), n_on


def subset(R, keep):
    idx = np.nonzero(keep)[0]
    n = len(idx)
    return {"n": n, "ref": R["ref"], "pos": np.ascontiguousarray(R["pos"][idx]), "cig_off": np.arange(n + 1, dtype=np.int64),
            "cig": np.ascontiguousarray(R["cig"][idx]), "seq_off": np.arange(n + 1, dtype=np.int64) * RL,
            "seq": np.ascontiguousarray(R["seq"].reshape(-1, RL)[idx].reshape(-1)), "qual": np.ascontiguousarray(R["qual"].reshape(-1, RL)[idx].reshape(-1)),
            "mapq": np.ascontiguousarray(R["mapq"][idx]), "rev": np.ascontiguousarray(R["rev"][idx])}


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def main():
    import torch
    import lofreq_amd as la
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bed_rate.json")
    R, target, text, n_on = make_bin()
    cs = np.concatenate([[0], np.cumsum(target, dtype=np.int64)])
    t0 = time.perf_counter()
    keep = (cs[R["pos"] + RL] - cs[R["pos"]]) > 0
    R_on = subset(R, keep)
    filter_ms = (time.perf_counter() - t0) * 1e3
    assert R_on["n"] == n_on
    cl = la.SnvCaller(0)
    cl.set_dense_strand_counts(False)
    dev = torch.device("cuda", 0)
    cap = 1 << 20
    d_counts = torch.zeros(TILE * 64, dtype=torch.uint8, device=dev)
    d_pvals = torch.zeros(cap * 128, dtype=torch.uint8, device=dev)
    bed = la.Bed.parse(text)
    hip = C.CDLL("libamdhip64.so")

    def n_obs(dt):
        t = dt._tracks()
        v = np.zeros(1, np.uint64)
        assert hip.hipMemcpy(C.c_void_p(v.ctypes.data), C.c_void_p(t.col_off + 8 * dt.ncols), C.c_size_t(8), 2) == 0
        return int(v[0])

    def road(reads, with_bed, host_mask):
        if with_bed:
            cl.set_bed(bed, "synth")
        t0 = time.perf_counter()
        rs = la.ReadSet.from_arrays(cl, reads)
        if with_bed:
            cl.set_bed(None)
        rs.baq(extended=True, idaq=False)
        dt = rs.pileup_snv(0, TILE)
        if host_mask:
            la.skip_snv_columns(cl, 1 - target[dt.col_pos])
        conf = la.VarcallConf()
        cl.snv_batch_device(dt, conf, d_counts, d_pvals, cap)
        st = cl.batch_finish()
        pv = d_pvals[: st.n_pvals * 128].cpu().numpy().view(la.COL_PVALS_DTYPE).copy()
        pv["col"] = dt.col_pos[pv["col"]]
        wall = (time.perf_counter() - t0) * 1e3
        bt = cl.baq_times()
        res = {"wall_ms": wall, "baq_ms": bt["ms_kernels"], "baq_reads": bt["n_reads"], "ncols": int(dt.ncols), "n_obs": n_obs(dt),
               "n_tested": int(st.n_tested), "n_pvals": int(st.n_pvals)}
        rs.close()
        return res, pv

    roads = {"a": (R, True, False), "b": (R_on, False, True), "b0": (R, False, True)}
    runs = {k: [] for k in roads}
    last = {}
    for p in range(PASSES + 1):                                 # pass 0 is the warm-up
        for k in (("a", "b", "b0") if p % 2 else ("b0", "b", "a")):
            res, pv = road(*roads[k])
            last[k] = pv
            if p:
                runs[k].append(res)

    def strip(pv):                                              # (the records come back in no fixed order)
        return sorted(zip(pv["col"].tolist(), pv["bonf"].tolist(), [x.tobytes() for x in pv["logp"]], [x.tobytes() for x in pv["status"]],
                          [x.tobytes() for x in pv["counts"]]))

    same = {k: strip(last[k]) == strip(last["a"]) for k in ("b", "b0")}
    out = {"shape": {"bin": TILE, "depth_on_targets": DEPTH, "read_len": RL, "reads": int(R["n"]), "reads_on_target": int(n_on),
                     "reads_off_target": int(R["n"] - n_on), "target_positions": int(target.sum()), "targets": text.count("\n")},
           "passes": PASSES, "caller_filter_host_ms": round(filter_ms, 1),
           "records_equal_a": same, "new_kernels_ms": "not measured"}
    for k, v in runs.items():
        out[k] = {"wall_ms": stats([r["wall_ms"] for r in v]), "baq_kernel_ms": stats([r["baq_ms"] for r in v]),
                  "baq_reads": v[0]["baq_reads"], "columns_to_count_kernel": v[0]["ncols"], "observations_to_count_kernel": v[0]["n_obs"],
                  "columns_tested": v[0]["n_tested"], "records": v[0]["n_pvals"]}
    json.dump(out, open(out_path, "w"), indent=1)
    print(json.dumps(out))
    bed.close()
    cl.close()


if __name__ == "__main__":
    main()
