"""BGZF blocks compressed on the device against zlib on the host -> profiles/bgzf_deflate_rate.json

  input      the payload of profiles/bgzf_rate.py: 400 000 C4-shaped records of 150 bases with block_size and core in front, a BAM
             body without a header, 3 750 blocks of 65280 bytes.  5 passes after a warm-up pass, medians (min - max).
  deflate    lfq_bgzf_deflate alone, input in pageable host memory: its three legs (lfq_last_bgzf_deflate_times: input + offsets
             down, the two kernels, sizes + blocks back), the kernels' GB/s of input, and the compressed size beside zlib level 1
             and level 6 on the same blocks
  chain      lfq_readset_encode_bam -> lfq_bam_frame_encoded -> lfq_bgzf_deflate of the framed body by pointer (taken from the
             device copy): wall time of each step and the deflate's legs
  host       zlib.compressobj (raw deflate, the same blocks) at level 1 and level 6, on 1 thread and on 16 threads -- the CPU
             budget of a job on the box

    python profiles/bgzf_deflate_rate.py [out.json]
"""
import ctypes as C
import gzip
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bgzf_rate as bz  # noqa: E402
import readset_from_bam_rate as rb  # noqa: E402

N_READS, PAYLOAD, REPS, THREADS = bz.N_READS, bz.PAYLOAD, bz.REPS, bz.THREADS
stats = bz.stats


def main():
    import lofreq_amd as la
    from lofreq_amd import _lib
    from lofreq_amd.pileup import bgzf_deflated_arrays
    L = _lib.load()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bgzf_deflate_rate.json")
    R = rb.make_records(N_READS)
    body_b = bz.bam_body(R)
    body = np.frombuffer(body_b, np.uint8).copy()
    chunks = [body_b[a:a + PAYLOAD] for a in range(0, len(body_b), PAYLOAD)]
    cl = la.SnvCaller(0)
    res = {"n_reads": N_READS, "record_bytes": int(R["record_bytes"]), "input_bytes": len(body), "n_blocks": len(chunks),
           "payload_per_block": PAYLOAD, "passes": REPS}
    # ---- lfq_bgzf_deflate alone
    legs = {k: [] for k in ("upload_ms", "kernels_ms", "download_ms", "wall_ms")}
    out = C.POINTER(_lib.BgzfDeflated)()
    for p in range(REPS + 1):
        t0 = time.perf_counter()
        rc = L.lfq_bgzf_deflate(cl.h, body.ctypes.data, len(body), None, 0, _lib.LFQ_BGZF_PUT_EOF, C.byref(out))
        wall = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and out.contents.n_blocks == len(chunks)
        t = la.last_bgzf_deflate_times(cl)
        if p:
            for k in ("upload_ms", "kernels_ms", "download_ms"):
                legs[k].append(t[k])
            legs["wall_ms"].append(wall)
    comp, comp_off, data_off, btype = bgzf_deflated_arrays(out.contents)
    assert gzip.decompress(comp.tobytes()) == body_b
    res["deflate"] = {k: stats(v) for k, v in legs.items()}
    res["deflate"]["kernels_input_GBps"] = len(body) / (np.median(legs["kernels_ms"]) * 1e-3) / 1e9
    res["deflate"]["upload_GBps"] = len(body) / (np.median(legs["upload_ms"]) * 1e-3) / 1e9
    res["deflate"]["download_GBps"] = len(comp) / (np.median(legs["download_ms"]) * 1e-3) / 1e9
    res["deflate"]["btype_counts"] = [int((btype == k).sum()) for k in range(3)]
    stream_bytes = int(len(comp) - 28 - 26 * len(chunks))

    # ---- zlib on the host: sizes and times
    def raw(level):
        def one(x):
            co = zlib.compressobj(level, zlib.DEFLATED, -15)
            return len(co.compress(x) + co.flush())
        return one

    def compress_all(level, threads):
        t0 = time.perf_counter()
        if threads == 1:
            n = sum(map(raw(level), chunks))
        else:
            with ThreadPoolExecutor(threads) as ex:
                n = sum(ex.map(raw(level), chunks, chunksize=16))
        return (time.perf_counter() - t0) * 1e3, n
    res["host_zlib"] = {}
    sizes = {}
    for level in (1, 6):
        for th in (1, THREADS):
            runs = [compress_all(level, th) for _ in range(REPS + 1)][1:]
            v = [r[0] for r in runs]
            sizes[level] = runs[0][1]
            res["host_zlib"]["level%d_%d_threads" % (level, th)] = dict(stats(v), input_GBps=len(body) / (np.median(v) * 1e-3) / 1e9)
    res["sizes"] = {"device_stream_bytes": stream_bytes, "zlib_level1_stream_bytes": int(sizes[1]), "zlib_level6_stream_bytes": int(sizes[6]),
                    "device_over_level1": stream_bytes / sizes[1], "device_over_level6": stream_bytes / sizes[6],
                    "device_ratio": stream_bytes / len(body)}

    # ---- the chain encode -> frame -> deflate
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
    walls = {k: [] for k in ("encode_ms", "frame_ms", "deflate_ms", "chain_ms")}
    dl = {k: [] for k in ("upload_ms", "kernels_ms", "download_ms")}
    enc, fr = C.POINTER(_lib.BamEncoded)(), C.POINTER(_lib.BamFramed)()
    for p in range(REPS + 1):
        t0 = time.perf_counter()
        assert L.lfq_readset_encode_bam(cl.h, h, C.byref(rc_), None, _lib.LFQ_BAM_PUT_ALIGNMENT, C.byref(enc)) == 0
        t1 = time.perf_counter()
        assert L.lfq_bam_frame_encoded(cl.h, cores.ctypes.data, N_READS, C.byref(fr)) == 0
        t2 = time.perf_counter()
        assert L.lfq_bgzf_deflate(cl.h, fr.contents.data, fr.contents.n_bytes, None, 0, _lib.LFQ_BGZF_PUT_EOF, C.byref(out)) == 0
        t3 = time.perf_counter()
        t = la.last_bgzf_deflate_times(cl)
        assert t["n_from_device"] == 1
        if p:
            for k, v in (("encode_ms", t1 - t0), ("frame_ms", t2 - t1), ("deflate_ms", t3 - t2), ("chain_ms", t3 - t0)):
                walls[k].append(v * 1e3)
            for k in dl:
                dl[k].append(t[k])
    framed = np.ctypeslib.as_array(C.cast(fr.contents.data, C.POINTER(C.c_uint8)), (int(fr.contents.n_bytes),))
    comp2 = bgzf_deflated_arrays(out.contents)[0]
    assert gzip.decompress(comp2.tobytes()) == framed.tobytes() and len(framed) == len(body)
    res["chain"] = dict({k: stats(v) for k, v in walls.items()}, deflate_legs_ms={k: stats(v) for k, v in dl.items()},
                        framed_bytes=int(len(framed)), compressed_bytes=int(len(comp2)), n_from_device=int(t["n_from_device"]),
                        body_equals_input=bool(framed.tobytes() == body_b))
    L.lfq_readset_destroy(h)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
