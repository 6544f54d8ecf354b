"""The .bai of a BAM built on the device against the same build on one host thread
-> profiles/bai_rate.json

  input      the payload of profiles/bgzf_rate.py and bgzf_deflate_rate.py: 400 000 C4-shaped records of 150 bases, framed by
             lfq_bam_frame_encoded and cut by lfq_bam_record_cuts into blocks of at most 65280 bytes that lfq_bgzf_deflate
             compresses.  5 passes after a warm-up pass, medians (min - max).
  device     lfq_bam_index_build on the resident framed body (n_from_device = 1): its legs (lfq_last_bam_index_times: tables down,
             the four kernels, the lists back -- on the device's clock --, the host's finishing pass) and the call's wall time
  host       lofreq_amd/csrc/lfq_bamidx_check.cpp --time: the same build from the header alone, as loops on one thread, on the
             same body and tables
  binary     where oracle/_ref/bin/lofreq is present: `lofreq index` of the written file (header blocks + body + marker), wall time

    python profiles/bai_rate.py [out.json]
"""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bgzf_rate as bz  # noqa: E402
import readset_from_bam_rate as rb  # noqa: E402
import bai_model as bm  # noqa: E402

N_READS, REPS = bz.N_READS, bz.REPS
stats = bz.stats
LOFREQ = os.path.join(ROOT, "oracle", "_ref", "bin", "lofreq")
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")


def main():
    import lofreq_amd as la
    from lofreq_amd import _lib
    from lofreq_amd.pileup import bgzf_deflated_arrays
    L = _lib.load()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bai_rate.json")
    R = rb.make_records(N_READS)
    body = np.frombuffer(bz.bam_body(R), np.uint8).copy()
    cl = la.SnvCaller(0)
    ref = R["ref"]
    rc_ = _lib.BamRecords()
    rc_.n_reads = N_READS
    n_cig, l_seq, l_name = np.ones(N_READS, np.uint32), np.full(N_READS, rb.RL, np.int32), np.full(N_READS, rb.L_QNAME, np.uint16)
    for k, v in (("data", R["data"]), ("data_off", R["data_off"]), ("pos", R["pos"]), ("flag", R["flag"]), ("mapq", R["mapq"]),
                 ("l_qname", l_name), ("n_cigar", n_cig), ("l_qseq", l_seq)):
        setattr(rc_, k, v.ctypes.data)
    rc_.ref = C.cast(C.c_char_p(ref), C.c_void_p)
    rc_.ref_len = len(ref)
    h = C.c_void_p()
    assert L.lfq_readset_create_from_bam(cl.h, C.byref(rc_), C.byref(h)) == 0
    cores = np.ascontiguousarray(body.reshape(N_READS, -1)[:, 4:36]).reshape(-1)
    enc, fr, out = C.POINTER(_lib.BamEncoded)(), C.POINTER(_lib.BamFramed)(), C.POINTER(_lib.BgzfDeflated)()
    assert L.lfq_readset_encode_bam(cl.h, h, C.byref(rc_), None, _lib.LFQ_BAM_PUT_ALIGNMENT, C.byref(enc)) == 0
    assert L.lfq_bam_frame_encoded(cl.h, cores.ctypes.data, N_READS, C.byref(fr)) == 0
    n_bytes = int(fr.contents.n_bytes)
    rec_off = np.ctypeslib.as_array(C.cast(fr.contents.rec_off, C.POINTER(C.c_int64)), (N_READS + 1,)).copy()
    t0 = time.perf_counter()
    cuts = la.bam_record_cuts(rec_off)
    cuts_ms = (time.perf_counter() - t0) * 1e3
    header = bm.header([("chr1", len(ref))])
    head_blocks = la.bgzf_deflate(cl, header)[0]
    assert L.lfq_bgzf_deflate(cl.h, fr.contents.data, n_bytes, cuts.ctypes.data, len(cuts), _lib.LFQ_BGZF_PUT_EOF, C.byref(out)) == 0
    comp, comp_off, data_off, _ = bgzf_deflated_arrays(out.contents)
    res = {"n_reads": N_READS, "body_bytes": n_bytes, "n_blocks": len(comp_off) - 1, "passes": REPS, "record_cuts_ms": cuts_ms}
    # ---- the device
    legs = {k: [] for k in ("upload_ms", "kernels_ms", "download_ms", "host_ms", "wall_ms")}
    bai = None
    for p in range(REPS + 1):
        t0 = time.perf_counter()
        idx = la.bam_index_build(cl, (fr.contents.data, n_bytes), rec_off, data_off, comp_off, len(head_blocks), 1)
        wall = (time.perf_counter() - t0) * 1e3
        t = la.last_bam_index_times(cl)
        assert t["n_from_device"] == 1 and t["n_recs"] == N_READS
        if p:
            for k in legs:
                legs[k].append(wall if k == "wall_ms" else t[k])
        bai = idx.to_bytes()
        idx.close()
    res["device"] = dict({k: stats(v) for k, v in legs.items()}, n_chunks=int(t["n_chunks"]), n_intervals=int(t["n_intervals"]),
                         n_launches=int(t["n_launches"]), bai_bytes=len(bai),
                         host_share_of_wall=float(np.median(legs["host_ms"]) / np.median(legs["wall_ms"])))
    # ---- one host thread: the header's loops
    framed = C.string_at(fr.contents.data, n_bytes)
    with tempfile.TemporaryDirectory() as tmp:
        cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        exe = os.path.join(tmp, "lfq_bamidx_check")
        subprocess.check_call([cxx, "-std=c++17", "-O3", "-I" + CSRC, os.path.join(CSRC, "lfq_bamidx_check.cpp"), "-o", exe])
        row = os.path.join(tmp, "row.bin")
        with open(row, "wb") as f:
            f.write(np.asarray([n_bytes, N_READS, len(comp_off) - 1, len(head_blocks), 1], np.int64).tobytes())
            f.write(rec_off.tobytes() + data_off.tobytes() + comp_off.tobytes() + framed)
        lines = subprocess.run([exe, "--time", row, str(REPS + 1)], check=True, capture_output=True, text=True).stdout.split("\n")
        ms = [float(x) for x in lines[1:REPS + 1]]
        assert bm.from_json(json.loads(lines[REPS + 1])) == bm.parse_bai(bai), "host and device disagree"
        res["host_one_thread"] = stats(ms)
        res["device_wall_over_host"] = float(np.median(legs["wall_ms"]) / np.median(ms))
        # ---- the reference's binary on the written file
        if os.path.exists(LOFREQ):
            path = os.path.join(tmp, "out.bam")
            open(path, "wb").write(head_blocks.tobytes() + comp.tobytes())
            ms = []
            for p in range(REPS + 1):
                t0 = time.perf_counter()
                subprocess.run([LOFREQ, "index", path], check=True, capture_output=True)
                ms.append((time.perf_counter() - t0) * 1e3)
            assert bm.parse_bai(open(path + ".bai", "rb").read()) == bm.parse_bai(bai), "the binary's index differs"
            res["lofreq_index_wall"] = dict(stats(ms[1:]), file_bytes=len(head_blocks) + len(comp))
    L.lfq_readset_destroy(h)
    json.dump(res, open(out_path, "w"))
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
