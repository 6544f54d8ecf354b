"""Rate of `lofreq indelqual` on the device -> profiles/indelqual_rate.json

  kernels    lfq_indelqual_batch on 400 000 and on 2 000 000 position-sorted reads of 150 bases (4 % with one insertion or
             deletion), Dindel and uniform mode: after a warm-up call, 7 calls each; device time of the call's kernels
             (lfq_last_indelqual_times: HIP events on their stream), their number, and the bytes they write per second against the
             6.29 TB/s copy ceiling of DESIGN.md section 3.  Bytes written: Dindel = one byte per base (BI and BD are one array) + the
             position table; uniform = two bytes per base.
  chain      reads -> VCF of a C4-shaped region (tests/golden_reads.py: 24 kb, 500x, planted indels, --call-indels) from host arrays,
             uploads included, two ways on the same build, alternating, 7 runs each after a warm-up pair:
               upload   BI / BD handed to lfq_readset_create as host arrays (the bytes `lofreq indelqual --dindel` writes)
               device   no BI / BD; lfq_readset_indelqual between the BAQ step and the indel pileup
             wall time from lfq_readset_create to the last record; both ways must write the same lines.
  reference  the first 100 000 of the 400 000 reads as SAM through `lofreq indelqual --dindel` of the 2.1.4 binary
             (oracle/_ref/bin/lofreq, where it exists), pinned to one core with taskset: wall time of the command (SAM in, BAM out)

    python profiles/indelqual_rate.py [out.json]
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
import golden_reads as gr  # noqa: E402

RL, REPS, N_REF, COPY_CEILING = 150, 7, 100000, 6.29e12


def make_reads(n, seed=41):
    """flat arrays: sorted starts at 500x over a random contig with a few long runs, 4 % of the reads with a 1..3 base indel"""
    rng = np.random.default_rng(seed)
    glen = n * RL // 500 + 1000
    g = rng.integers(0, 4, glen).astype(np.uint8)
    for s in rng.integers(0, glen - 40, glen // 400):
        g[s:s + int(rng.integers(4, 26))] = g[s]
    ref = np.frombuffer(b"ACGT", np.uint8)[g].tobytes()
    pos = np.sort(rng.integers(0, glen - RL - 8, n)).astype(np.int32)
    kind = rng.random(n)
    a = rng.integers(10, RL - 20, n)
    l = rng.integers(1, 4, n)
    ncig = np.where(kind < 0.04, 3, 1)
    cig_off = np.zeros(n + 1, np.int64)
    np.cumsum(ncig, out=cig_off[1:])
    cig = np.empty(int(cig_off[-1]), np.uint32)
    plain = kind >= 0.04
    cig[cig_off[:-1][plain]] = RL << 4
    ins = kind < 0.02
    dele = (kind >= 0.02) & (kind < 0.04)
    for m, op in ((ins, 1), (dele, 2)):
        o = cig_off[:-1][m]
        cig[o] = a[m] << 4
        cig[o + 1] = (l[m] << 4) | op
        cig[o + 2] = (RL - a[m] - (l[m] if op == 1 else 0)) << 4
    return {"n": n, "ref": ref, "pos": pos, "cig_off": cig_off, "cig": cig, "seq_off": np.arange(n + 1, dtype=np.int64) * RL}


def packed(R, _lib):
    rd = _lib.BaqReads()
    rd.n_reads = R["n"]
    rd.pos, rd.cigar_off, rd.cigar, rd.seq_off = (R[k].ctypes.data for k in ("pos", "cig_off", "cig", "seq_off"))
    rd.ref = C.cast(C.c_char_p(R["ref"]), C.c_void_p)
    rd.ref_len = len(R["ref"])
    return rd


def stats(v):
    return {"min": float(min(v)), "median": float(np.median(v)), "all": [round(float(x), 4) for x in sorted(v)]}


def kernel_rates(cl, _lib, iq):
    out = []
    for n in (400000, 2000000):
        R = make_reads(n)
        rd = packed(R, _lib)
        nb = n * RL
        bi, bd = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8)
        for mode, conf in (("dindel", iq.make_conf("dindel")), ("uniform", iq.make_conf("uniform", 40, 45))):
            ms, wall = [], []
            for i in range(REPS + 1):
                t0 = time.perf_counter()
                _lib.check(_lib.load().lfq_indelqual_batch(cl.h, C.byref(rd), C.byref(conf), bi.ctypes.data, bd.ctypes.data))
                t1 = time.perf_counter()
                t = iq.last_times(cl)
                if i:
                    ms.append(t["ms_kernels"])
                    wall.append((t1 - t0) * 1e3)
            written = nb + len(R["ref"]) if mode == "dindel" else 2 * nb
            k = stats(ms)
            out.append({"n_reads": n, "read_length": RL, "mode": mode, "n_launches": t["n_launches"], "bytes_written": written,
                        "kernel_ms": k, "bytes_per_s_at_min": written / (k["min"] * 1e-3),
                        "share_of_copy_ceiling_at_min": written / (k["min"] * 1e-3) / COPY_CEILING,
                        "floor_ms_at_copy_ceiling": written / COPY_CEILING * 1e3,
                        "call_wall_ms_with_fetch_to_host": stats(wall)})
    return out


def chain(la, cl, R, kw, device_idq):
    t0 = time.perf_counter()
    rs = la.ReadSet.from_arrays(cl, R)
    rs.baq(extended=True, idaq=True)
    if device_idq:
        rs.indelqual("dindel")
    conf = la.VarcallConf(**kw)
    cols, col_pos = rs.pileup_indels(0, R["glen"])
    irecs, _ = la.call_indels(cl, cols, conf)
    dt = rs.pileup_snv(0, R["glen"])
    la.skip_snv_columns(cl, cols.cons_indel)
    recs, _, _ = cl.call_snvs(dt, conf)
    ms = (time.perf_counter() - t0) * 1e3
    rs.close()
    return ms, irecs.tobytes() + recs.tobytes()


def chain_rates(la, cl, _lib, iq):
    params = dict(seed=603, glen=24000, depth_lo=500, depth_hi=500, min_q=6, snv_every=60, indel_every=240)
    R = gr.make(**params)
    R["bi"] = R["bd"] = None
    R["flags"] = np.zeros(R["n"], np.uint8)
    Rp = {"n": R["n"], "ref": R["ref"], "pos": R["pos"], "cig_off": R["cig_off"], "cig": R["cig"], "seq_off": R["seq_off"]}
    nb = int(R["seq_off"][-1])
    bi, bd = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8)
    conf = iq.make_conf("dindel")
    rd = packed(Rp, _lib)
    _lib.check(_lib.load().lfq_indelqual_batch(cl.h, C.byref(rd), C.byref(conf), bi.ctypes.data, bd.ctypes.data))
    U = dict(R, bi=bi, bd=bd, flags=np.full(R["n"], 3, np.uint8))
    kw = {"flag": 3 | 8}
    t_up, t_dev, same = [], [], True
    for i in range(REPS + 1):
        a, ra = chain(la, cl, U, kw, False)
        b, rb = chain(la, cl, R, kw, True)
        same = same and ra == rb
        if i:
            t_up.append(a)
            t_dev.append(b)
    return {"shape": params, "n_reads": int(R["n"]), "n_bases": nb, "same_records_both_ways": bool(same),
            "upload_route_ms": stats(t_up), "device_route_ms": stats(t_dev)}


def reference_rate():
    binary = os.path.join(ROOT, "oracle", "_ref", "bin", "lofreq")
    if not os.path.exists(binary):
        return None
    R = make_reads(400000)
    ref = R["ref"].decode()
    seq, qual = "A" * RL, "I" * RL
    ops = "MIDNSHP=X"
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.fa"), "w").write(">chr1\n" + ref + "\n")
        with open(os.path.join(tmp, "t.sam"), "w") as f:
            f.write("@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:chr1\tLN:%d\n" % len(ref))
            for i in range(N_REF):
                cg = "".join("%d%s" % (int(w) >> 4, ops[int(w) & 15]) for w in R["cig"][R["cig_off"][i]:R["cig_off"][i + 1]])
                f.write("r%d\t0\tchr1\t%d\t60\t%s\t*\t0\t0\t%s\t%s\n" % (i, int(R["pos"][i]) + 1, cg, seq, qual))
        subprocess.check_call([binary, "faidx", "t.fa"], cwd=tmp)
        t0 = time.perf_counter()
        subprocess.run(["taskset", "-c", "0", binary, "indelqual", "--dindel", "-f", "t.fa", "-o", "out.bam", "t.sam"], cwd=tmp,
                       check=True, capture_output=True)
        s = time.perf_counter() - t0
    return {"n_reads": N_REF, "wall_s": s, "us_per_read": s * 1e6 / N_REF}


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("indelqual_rate: no GPU; rates are measured on the device only")
    import lofreq_amd as la
    from lofreq_amd import _lib, indelqual as iq
    cl = la.SnvCaller(0)
    out = {"copy_ceiling_bytes_per_s": COPY_CEILING, "kernels": kernel_rates(cl, _lib, iq), "chain": chain_rates(la, cl, _lib, iq)}
    cl.close()
    ref = reference_rate()
    if ref:
        out["reference_binary_one_core"] = ref
        k = [x for x in out["kernels"] if x["mode"] == "dindel" and x["n_reads"] == 400000][0]
        out["speedup_per_read_call_wall"] = ref["us_per_read"] / (k["call_wall_ms_with_fetch_to_host"]["median"] * 1e3 / k["n_reads"])
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
