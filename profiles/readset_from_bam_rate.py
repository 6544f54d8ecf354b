"""BAM records decoded on the device against the per-base host loop
-> profiles/readset_from_bam_rate.json

  roads      one region of 100 000 and one of 2 000 000 position-sorted C4-shaped records (150 bases at 500x, 24-byte name, one
             CIGAR operation, NM / MD / AS and BI / BD Z tags: 576 bytes of bam1_t.data a read), through the region binding, two
             ways on the same build, alternating, 5 passes each after a warm-up pass (profiles/readset_from_bam_harness.c):
               (a) arrays    two bam_aux_get walks + lfq_region_add_read per record (its loop unpacks the bases on the calling
                             thread) -> lfq_region_end -> lfq_readset_create
               (b) records   lfq_region_add_record per record -> lfq_region_end -> lfq_readset_create_from_bam
             LFQ_SYNC_UPLOAD=1, so that lfq_readset_create returns when its copies have landed and both roads end at the same
             point.  Wall time from lfq_region_begin until lfq_region_end has returned, and the add loop's share of it (the time the
             caller's thread spends on the records), median / min / max / all passes.
  legs   (c) lfq_last_bam_decode_times of road (b)'s last pass: the record upload and the per-base download against the 63 GB/s
             of the link (PCIe Gen5 x16), and -- from one more pass under `rocprofv3 --kernel-trace --stats` in a child process of
             its own -- the base kernel's bytes moved (read: 4-bit bases, qualities, BI, BD strings and 24 descriptor bytes a read;
             written: four per-base arrays) per second against the 6.29 TB/s copy ceiling of DESIGN.md section 0.

    python profiles/readset_from_bam_rate.py [out.json]
"""
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["LFQ_SYNC_UPLOAD"] = "1"

RL, DEPTH, REPS, COPY_CEILING, LINK = 150, 500, 5, 6.29e12, 63e9
SIZES = (100000, 2000000)
L_QNAME = 24


def make_records(n, seed=811):
    """n records of one shape as a [n, record bytes] array -> the arrays of an lfq_bam_records"""
    rng = np.random.default_rng(seed)
    fields = [np.zeros((n, L_QNAME), np.uint8),
              np.tile(np.frombuffer(np.asarray([RL << 4], "<u4").tobytes(), np.uint8), (n, 1)),
              ((1 << rng.integers(0, 4, (n, RL // 2))) << 4 | (1 << rng.integers(0, 4, (n, RL // 2)))).astype(np.uint8),    # A C G T
              rng.integers(2, 42, (n, RL), dtype=np.uint8),
              np.tile(np.frombuffer(b"NMC\x01MDZ150\x00ASC\x96BIZ", np.uint8), (n, 1)),
              (33 + rng.integers(0, 60, (n, RL), dtype=np.uint8)).astype(np.uint8), np.tile(np.frombuffer(b"\x00BDZ", np.uint8), (n, 1)),
              (33 + rng.integers(0, 60, (n, RL), dtype=np.uint8)).astype(np.uint8), np.zeros((n, 1), np.uint8)]
    name = np.frombuffer(b"read", np.uint8)
    fields[0][:, :4] = name
    data = np.ascontiguousarray(np.concatenate(fields, axis=1))
    size = data.shape[1]
    glen = n * RL // DEPTH + RL
    return {"n": n, "record_bytes": size, "data": data.reshape(-1), "data_off": np.arange(n + 1, dtype=np.int64) * size,
            "pos": (np.arange(n, dtype=np.int64) * RL // DEPTH).astype(np.int32), "flag": ((np.arange(n) & 1) << 4).astype(np.uint16),
            "mapq": np.full(n, 60, np.uint8), "ref": rng.choice(np.frombuffer(b"ACGT", np.uint8), glen).tobytes()}


def stats(v):
    return {"min": float(min(v)), "median": float(np.median(v)), "max": float(max(v)), "all": [round(float(x), 3) for x in sorted(v)]}


def build_harness(tmp):
    lib = os.path.join(tmp, "libreadset_from_bam_harness.so")
    subprocess.run(["gcc", "-std=gnu99", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "integration"), os.path.join(ROOT, "profiles", "readset_from_bam_harness.c"),
                    os.path.join(ROOT, "integration", "lofreq_amd_region.c"), "-L" + os.path.join(ROOT, "lofreq_amd"), "-llofreq_amd",
                    "-Wl,-rpath," + os.path.join(ROOT, "lofreq_amd"), "-o", lib], check=True, capture_output=True, text=True)
    H = C.CDLL(lib)
    vp = C.c_void_p
    H.lfq_prof_road.argtypes = [vp, vp, C.c_int, C.c_int64, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int64,
                                C.c_int, vp, vp]
    return H


def run_road(H, la, cl, R, road, passes):
    conf = la.VarcallConf()
    add, total = np.zeros(passes), np.zeros(passes)
    rc = H.lfq_prof_road(cl.h, C.addressof(conf.c), road, R["n"], R["data"].ctypes.data, R["data_off"].ctypes.data,
                         R["pos"].ctypes.data, R["flag"].ctypes.data, R["mapq"].ctypes.data, L_QNAME, 1, RL, R["ref"], len(R["ref"]),
                         passes, add.ctypes.data, total.ctypes.data)
    if rc != 0:
        raise SystemExit("readset_from_bam_rate: road %d failed with %d" % (road, rc))
    return add, total


def roads(H, la, cl):
    out = []
    for n in SIZES:
        R = make_records(n)
        nb = n * RL
        run_road(H, la, cl, R, 0, 1), run_road(H, la, cl, R, 1, 1)                  # warm-up: context buffers, pinned pools
        a_add, a_tot, b_add, b_tot, legs = [], [], [], [], []
        for _ in range(REPS):                                                       # alternating; pass 0 of each call re-pins the
            x = run_road(H, la, cl, R, 0, 2)                                        # binding's own buffers and is dropped
            y = run_road(H, la, cl, R, 1, 2)
            a_add.append(x[0][1]), a_tot.append(x[1][1]), b_add.append(y[0][1]), b_tot.append(y[1][1])
            legs.append(la.last_bam_decode_times(cl))
        a, b = stats(a_tot), stats(b_tot)
        t = legs[-1]
        down = nb * 4
        out.append({"n_reads": n, "n_bases": nb, "record_bytes_per_read": R["record_bytes"],
                    "a_arrays_ms": a, "a_add_loop_ms": stats(a_add), "b_records_ms": b, "b_add_loop_ms": stats(b_add),
                    "a_spread_ms": a["max"] - a["min"],
                    "b_not_slower_beyond_a_spread": bool(b["median"] <= a["median"] + (a["max"] - a["min"])),
                    "link_bytes": {"a_down": nb * 4 + n * (4 + 8 + 8 + 4 + 3), "b_down": int(t["n_data_bytes"]) + n * 24 + n * (4 + 8 + 8 + 4 + 3),
                                   "b_up": down + n},
                    "c_decode_times_last_pass": t,
                    "c_upload_ms": stats([l["upload_ms"] for l in legs]), "c_kernels_ms_aux_and_base": stats([l["kernels_ms"] for l in legs]),
                    "c_download_ms": stats([l["download_ms"] for l in legs]),
                    "c_upload_share_of_link": (t["n_data_bytes"] + n * 24) / (np.median([l["upload_ms"] for l in legs]) * 1e-3) / LINK,
                    "c_download_share_of_link": down / (np.median([l["download_ms"] for l in legs]) * 1e-3) / LINK})
    return out


def one_pass():
    """the child under rocprofv3: two direct lfq_readset_create_from_bam calls on the large size"""
    import lofreq_amd as la
    cl = la.SnvCaller(0)
    R = make_records(SIZES[-1])
    lq, nc, ls = np.full(R["n"], L_QNAME, np.uint16), np.ones(R["n"], np.uint32), np.full(R["n"], RL, np.int32)
    for _ in range(2):
        rs = la.ReadSet.from_bam_records(cl, R["data"], R["data_off"], R["pos"], R["flag"], R["mapq"], lq, nc, ls, R["ref"])
        rs.close()
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
    n = SIZES[-1]
    nb = n * RL
    out = {"n_reads": n, "passes_in_the_trace": 2}
    for key, name in (("aux", "lfq_bam_aux_kernel"), ("bases", "lfq_bam_bases_kernel")):
        hit = [r for r in rows if name in r.get("Name", "")]
        out[key] = hit[0] if hit else None
    if out["bases"] and out["bases"].get("MinNs"):
        read, written = nb // 2 + 3 * nb + 24 * n, 4 * nb
        for which in ("MinNs", "MaxNs"):
            ns = float(out["bases"][which])
            out["bases_bytes_per_s_at_%s" % which] = (read + written) / (ns * 1e-9)
            out["bases_share_of_copy_ceiling_at_%s" % which] = (read + written) / (ns * 1e-9) / COPY_CEILING
        out["bases_bytes_moved"] = read + written
    return out


def main():
    if "--one-pass" in sys.argv:
        return one_pass()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("readset_from_bam_rate: no GPU; rates are measured on the device only")
    import lofreq_amd as la
    with tempfile.TemporaryDirectory() as tmp:
        H = build_harness(tmp)
        cl = la.SnvCaller(0)
        out = {"copy_ceiling_bytes_per_s": COPY_CEILING, "link_bytes_per_s": LINK, "roads": roads(H, la, cl)}
        cl.close()
    if "--no-trace" not in sys.argv:
        out["kernels"] = kernel_trace()
    text = json.dumps(out, indent=1)
    print(text)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if args:
        open(args[0], "w").write(text + "\n")


if __name__ == "__main__":
    main()
