"""Rate of the viterbi realigner: 100 000 reads of 150 bases, every one with one indel.

  device     lfq_viterbi_batch on the whole batch: after a warm-up call, median of 10 calls of the wall time of the call and of
             the device time of its kernels (lfq_last_viterbi_times: HIP events on their stream)
  reference  the first 10 000 of the same reads as SAM through `lofreq viterbi` of the 2.1.4 binary (oracle/_ref/bin/lofreq),
             pinned to one core with taskset, wall time of the command (it reads SAM and writes BAM; no other work)

    python profiles/viterbi_rate.py [out.json]      (prints the JSON; cells = 3 (q + 1) (w + 1) per realigned read)
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import viterbi_reads as vr  # noqa: E402

N_READS, N_REF, RL, GLEN, REPS = 100000, 10000, 150, 60000, 10


def make_reads(seed=31):
    rng = np.random.default_rng(seed)
    genome = vr.make_genome(rng, GLEN).upper().replace("N", "A")
    reads = []
    for r in range(N_READS):
        p = int(rng.integers(10, GLEN - RL - 50))
        a = int(rng.integers(8, RL - 16))
        l = int(rng.integers(1, 4))
        if r % 2:
            seq = genome[p:p + a] + genome[p + a + l:p + RL + l]
            cig = [("M", a), ("D", l), ("M", RL - a)]
        else:
            seq = genome[p:p + a] + "".join(rng.choice(list("ACGT"), l)) + genome[p + a:p + RL - l]
            cig = [("M", a), ("I", l), ("M", RL - a - l)]
        reads.append({"name": "r%d" % r, "pos0": p, "cigar": cig, "seq": seq, "qual": [int(v) for v in rng.integers(20, 42, RL)]})
    return genome, reads


def main():
    import lofreq_amd as la
    from lofreq_amd import _lib, viterbi as lv
    genome, reads = make_reads()
    rd, keep = lv.pack_reads([vr.lib_read(r) for r in reads], genome.encode())
    cl = la.SnvCaller(0)
    L = _lib.load()
    res = C.POINTER(_lib.ViterbiResult)()
    wall, dev = [], []
    for i in range(REPS + 1):
        t0 = time.perf_counter()
        _lib.check(L.lfq_viterbi_batch(cl.h, C.byref(rd), -1, C.byref(res)), "lfq_viterbi_batch")
        t1 = time.perf_counter()
        t = lv.last_times(cl)
        if i:
            wall.append((t1 - t0) * 1e3)
            dev.append(t["ms_kernels"])
    per_read = []
    for r in reads:
        q = sum(l for o, l in r["cigar"] if o in "MI")
        x = r["pos0"] + sum(l for o, l in r["cigar"] if o in "MD")
        w = min(len(genome), x + 10) - max(0, r["pos0"] - 10)
        per_read.append(3 * (q + 1) * (w + 1))
    cells = sum(per_read)
    out = {"n_reads": N_READS, "read_length": RL, "n_realigned": t["n_realigned"], "n_launches": t["n_launches"],
           "cells": cells, "device_ms": sorted(dev), "wall_ms": sorted(wall),
           "device_ms_median": float(np.median(dev)), "wall_ms_median": float(np.median(wall))}
    out["device_cells_per_s"] = cells / (out["device_ms_median"] * 1e-3)
    out["wall_us_per_read"] = out["wall_ms_median"] * 1e3 / N_READS
    cl.close()
    binary = os.path.join(ROOT, "oracle", "_ref", "bin", "lofreq")
    if os.path.exists(binary):
        with tempfile.TemporaryDirectory() as tmp:
            open(os.path.join(tmp, "t.fa"), "w").write(">chr1\n" + genome + "\n")
            open(os.path.join(tmp, "t.sam"), "w").write(vr.sam_text(genome, reads[:N_REF]))
            subprocess.check_call([binary, "faidx", "t.fa"], cwd=tmp)
            t0 = time.perf_counter()
            subprocess.run(["taskset", "-c", "0", binary, "viterbi", "-f", "t.fa", "-o", "out.bam", "t.sam"], cwd=tmp, check=True,
                           capture_output=True)
            ref_s = time.perf_counter() - t0
        out["reference_n_reads"] = N_REF
        out["reference_wall_s"] = ref_s
        out["reference_us_per_read"] = ref_s * 1e6 / N_REF
        out["reference_cells_per_s"] = sum(per_read[:N_REF]) / ref_s
        out["speedup_per_read_wall"] = out["reference_us_per_read"] / out["wall_us_per_read"]
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
