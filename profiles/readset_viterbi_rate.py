"""The realigner as a step of the resident read set against the host road
-> profiles/readset_viterbi_rate.json

  roads      100 000 and 400 000 position-sorted reads of 150 bases at 500x with the planted indels of the C4-shaped golden
             (tests/golden_reads.py, indel_every = 240), from host arrays to a realigned, re-sorted read set that is ready for
             BAQ, two ways on the same build, alternating, 7 runs each after a warm-up pair:
               host      lfq_viterbi_batch -> stable argsort of the new positions -> repack (numpy, vectorised) ->
                         lfq_readset_create
               resident  lfq_readset_create -> lfq_readset_viterbi
             LFQ_SYNC_UPLOAD=1, so that lfq_readset_create returns when its copies have landed and both roads end at the
             same point.  Wall time (median, min, all runs), ms_kernels of the realignment (lfq_last_viterbi_times), and the
             bytes that cross the link on each road, computed from the array sizes.
  kernels    one resident pass over the 400 000 reads under `rocprofv3 --kernel-trace --stats` in a child process of its own:
             the times of lfq_vit_gather_kernel and lfq_readset_permute_kernel, the permute kernel's bytes (read + written)
             per second against the 6.29 TB/s copy ceiling of DESIGN.md section 0.

    python profiles/readset_viterbi_rate.py [out.json]
"""
import csv
import glob
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
os.environ["LFQ_SYNC_UPLOAD"] = "1"
import golden_reads as gr  # noqa: E402

RL, REPS, COPY_CEILING = 150, 7, 6.29e12
SIZES = (100000, 400000)


def make_reads(n):
    R = gr.make(seed=603, glen=n * RL // 500, depth_lo=500, depth_hi=500, min_q=6, snv_every=60, indel_every=240)
    R = dict(R, bi=None, bd=None, lb=None)
    R["flags"] = np.zeros(R["n"], np.uint8)
    return R


def stats(v):
    return {"min": float(min(v)), "median": float(np.median(v)), "max": float(max(v)), "all": [round(float(x), 3) for x in sorted(v)]}


def host_road(la, lv, _lib, cl, R):
    import ctypes as C
    t0 = time.perf_counter()
    rd = _lib.BaqReads()
    rd.n_reads = int(R["n"])
    rd.pos, rd.cigar_off, rd.cigar = R["pos"].ctypes.data, R["cig_off"].ctypes.data, R["cig"].ctypes.data
    rd.seq_off, rd.seq, rd.qual = R["seq_off"].ctypes.data, R["seq"].ctypes.data, R["qual"].ctypes.data
    rd.ref = C.cast(C.c_char_p(R["ref"]), C.c_void_p)
    rd.ref_len = len(R["ref"])
    pos, status, cig_off, cig = lv.viterbi_arrays(cl, rd, -1)
    t = lv.last_times(cl)
    n = int(R["n"])
    order = np.argsort(pos, kind="stable")
    so = R["seq_off"]
    lens, clens = np.diff(so)[order], np.diff(cig_off)[order]
    new_so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    new_co = np.concatenate([[0], np.cumsum(clens)]).astype(np.int64)
    base_idx = np.repeat(so[:-1][order] - new_so[:-1], lens) + np.arange(int(new_so[-1]))
    cig_idx = np.repeat(cig_off[:-1][order] - new_co[:-1], clens) + np.arange(int(new_co[-1]))
    N = dict(R, pos=pos[order], cig=cig[cig_idx], cig_off=new_co, seq_off=new_so, seq=R["seq"][base_idx], qual=R["qual"][base_idx],
             mapq=R["mapq"][:n][order], rev=R["rev"][:n][order], flags=R["flags"][:n][order])
    rs = la.ReadSet.from_arrays(cl, N)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, t, rs, (pos, status, cig_off, cig)


def resident_road(la, lv, cl, R):
    t0 = time.perf_counter()
    rs = la.ReadSet.from_arrays(cl, R)
    new, result, order = rs.viterbi(-1)
    ms = (time.perf_counter() - t0) * 1e3
    t = lv.last_times(cl)
    rs.close()
    return ms, t, new, result


def link_bytes(R, result):
    """bytes over the link on each road, from the array sizes (lfq_viterbi.hip: 48-byte descriptor, 16-byte outcome, 128-byte
    transition table per distinct window length, 1504 bytes of emissions; per realigned read q + w state bytes come back)"""
    pos, status, cig_off, cig = result
    n, nb = int(R["n"]), int(R["seq_off"][-1])
    re = np.flatnonzero((status & 7) == 3)
    q_total = w_total = 0
    widths = set()
    for r in re:
        w = R["cig"][R["cig_off"][r]:R["cig_off"][r + 1]]
        op, ln = w & 15, (w >> 4).astype(np.int64)
        q = int(ln[(op == 0) | (op == 1) | (op == 7) | (op == 8)].sum())
        x = int(R["pos"][r]) + int(ln[(op == 0) | (op == 2) | (op == 7) | (op == 8)].sum())
        wl = min(x + 10, len(R["ref"])) - max(int(R["pos"][r]) - 10, 0)
        q_total, w_total = q_total + q, w_total + wl
        widths.add(wl)
    nw = len(re)
    tables = 128 * len(widths) + 1504
    create = lambda ncig, per_base: n * 4 + 2 * (n + 1) * 8 + ncig * 4 + len(R["ref"]) + 3 * n + (2 * nb if per_base else 0)
    states_back = q_total + w_total + 16 * nw
    host = {"viterbi_down": 48 * nw + tables + 2 * q_total + w_total, "viterbi_up": states_back,
            "readset_create_down": create(int(cig_off[-1]), True)}
    resident = {"readset_create_down": create(int(R["cig_off"][-1]), True), "viterbi_down": (48 + 16) * nw + tables,
                "viterbi_up": states_back, "new_set_down": create(int(cig_off[-1]), False) + 8 * n}
    return {"n_realigned": nw, "host": dict(host, total=sum(host.values())), "resident": dict(resident, total=sum(resident.values()))}


def roads(la, lv, _lib, cl):
    out = []
    for n in SIZES:
        R = make_reads(n)
        t_host, t_res, k_host, k_res, same = [], [], [], [], True
        result = None
        for i in range(REPS + 1):
            a, ta, rs_a, res_a = host_road(la, lv, _lib, cl, R)
            rs_a.close()
            b, tb, rs_b, res_b = resident_road(la, lv, cl, R)
            rs_b.close()
            same = same and all(np.array_equal(x, y) for x, y in zip(res_a, res_b))
            result = res_a
            if i:
                t_host.append(a), t_res.append(b), k_host.append(ta["ms_kernels"]), k_res.append(tb["ms_kernels"])
        h, r = stats(t_host), stats(t_res)
        out.append({"n_reads": int(R["n"]), "n_bases": int(R["seq_off"][-1]), "same_result_both_roads": bool(same),
                    "host_road_ms": h, "resident_road_ms": r, "host_road_spread_ms": h["max"] - h["min"],
                    "resident_not_slower_beyond_host_spread": bool(r["median"] <= h["median"] + (h["max"] - h["min"])),
                    "ms_kernels_host_road": stats(k_host), "ms_kernels_resident_road_with_gather": stats(k_res),
                    "link_bytes": link_bytes(R, result)})
    return out


def one_pass():
    """the child under rocprofv3: a warm-up and one resident pass over the large size"""
    import lofreq_amd as la
    from lofreq_amd import viterbi as lv
    cl = la.SnvCaller(0)
    R = make_reads(SIZES[-1])
    for _ in range(2):
        _, _, new, _ = resident_road(la, lv, cl, R)
        new.close()
    cl.close()


def kernel_trace():
    tool = "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return {"error": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([tool, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                            os.path.abspath(__file__), "--one-pass"], capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            return {"error": "rocprofv3 exit %d" % p.returncode, "stderr": p.stderr[-1500:]}
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            rows += list(csv.DictReader(open(path)))
    nb = SIZES[-1] * RL
    out = {"n_reads": SIZES[-1], "passes_in_the_trace": 2}
    for key, name in (("gather", "lfq_vit_gather_kernel"), ("permute", "lfq_readset_permute_kernel"), ("viterbi", "lfq_viterbi_kernel")):
        hit = [r for r in rows if name in r.get("Name", "")]
        out[key] = hit[0] if hit else None
    if out["permute"] and out["permute"].get("MinNs"):
        ns = float(out["permute"]["MinNs"])
        moved = 2 * 2 * nb                                      # seq + qual, read and written
        out["permute_bytes_moved"] = moved
        out["permute_bytes_per_s_at_min"] = moved / (ns * 1e-9)
        out["permute_share_of_copy_ceiling_at_min"] = moved / (ns * 1e-9) / COPY_CEILING
    return out


def main():
    if "--one-pass" in sys.argv:
        return one_pass()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("readset_viterbi_rate: no GPU; rates are measured on the device only")
    import lofreq_amd as la
    from lofreq_amd import _lib, viterbi as lv
    cl = la.SnvCaller(0)
    out = {"copy_ceiling_bytes_per_s": COPY_CEILING, "roads": roads(la, lv, _lib, cl)}
    cl.close()
    out["kernels"] = kernel_trace()
    text = json.dumps(out, indent=1)
    print(text)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if args:
        open(args[0], "w").write(text + "\n")


if __name__ == "__main__":
    main()
