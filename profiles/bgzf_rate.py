"""BGZF blocks inflated on the device against zlib on the host -> profiles/bgzf_rate.json

  input      400 000 C4-shaped records of 150 bases (profiles/readset_from_bam_rate.py::make_records: 576 bytes of bam1_t.data a
             read) with block_size and core in front, as a BAM body without a header, in BGZF blocks of 65280 payload bytes written
             by zlib at level 6.  5 passes after a warm-up pass, medians (min - max).
  inflate    lfq_bgzf_inflate alone: its three legs (lfq_last_bgzf_times: compressed bytes + descriptors down, the kernel, statuses
             + inflated bytes back) and the kernel's inflated GB/s
  roads      lfq_readset_create_from_bgzf (inflate + scan + decode from the device copy) against lfq_readset_create_from_bam on the
             same records already inflated (pageable memory): wall time, the bytes each road sends down the link, and
             n_decodes_from_device
  host       zlib.decompress (raw deflate, the same blocks) on 1 thread and on 16 threads -- the CPU budget of a job on the box

    python profiles/bgzf_rate.py [out.json]
"""
import ctypes as C
import json
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import readset_from_bam_rate as rb  # noqa: E402

N_READS, PAYLOAD, LEVEL, REPS, THREADS = 400000, 65280, 6, 5, 16


def bam_body(R):
    """the records of make_records as they lie in a file: block_size | 32-byte core | data"""
    n, size = R["n"], R["record_bytes"]
    core = np.zeros((n, 36), np.uint8)
    head = np.zeros(n, np.dtype([("bs", "<i4"), ("tid", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                                 ("n_cig", "<u2"), ("flag", "<u2"), ("l_seq", "<i4"), ("mtid", "<i4"), ("mpos", "<i4"), ("tlen", "<i4")]))
    head["bs"], head["tid"], head["pos"], head["l_name"], head["mapq"] = 32 + size, 0, R["pos"], rb.L_QNAME, R["mapq"]
    head["bin"], head["n_cig"], head["flag"], head["l_seq"], head["mtid"], head["mpos"] = 4680, 1, R["flag"], rb.RL, -1, -1
    core[:] = head.view(np.uint8).reshape(n, 36)
    return np.concatenate([core, R["data"].reshape(n, size)], axis=1).reshape(-1).tobytes()


def bgzf(payload):
    out, raws = [], []
    for a in range(0, len(payload), PAYLOAD):
        chunk = payload[a:a + PAYLOAD]
        co = zlib.compressobj(LEVEL, zlib.DEFLATED, -15)
        raw = co.compress(chunk) + co.flush()
        raws.append(raw)
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(raw) + 8 - 1) + raw
                   + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    return b"".join(out), raws


def stats(v):
    return {"min": float(min(v)), "median": float(np.median(v)), "max": float(max(v)), "all": [round(float(x), 3) for x in sorted(v)]}


def main():
    import lofreq_amd as la
    from lofreq_amd import _lib
    L = _lib.load()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bgzf_rate.json")
    R = rb.make_records(N_READS)
    body = bam_body(R)
    comp_b, raws = bgzf(body)
    comp = np.frombuffer(comp_b, np.uint8).copy()
    cl = la.SnvCaller(0)
    res = {"n_reads": N_READS, "record_bytes": int(R["record_bytes"]), "inflated_bytes": len(body), "compressed_bytes": len(comp),
           "n_blocks": len(raws), "payload_per_block": PAYLOAD, "zlib_level": LEVEL, "passes": REPS}
    # ---- lfq_bgzf_inflate alone
    legs = {k: [] for k in ("upload_ms", "kernels_ms", "download_ms", "wall_ms")}
    r = C.POINTER(_lib.BgzfResult)()
    for p in range(REPS + 1):
        t0 = time.perf_counter()
        rc = L.lfq_bgzf_inflate(cl.h, comp.ctypes.data, len(comp), C.byref(r))
        wall = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and r.contents.n_bytes == len(body)
        t = la.last_bgzf_times(cl)
        if p:
            for k in ("upload_ms", "kernels_ms", "download_ms"):
                legs[k].append(t[k])
            legs["wall_ms"].append(wall)
    got = np.ctypeslib.as_array(C.cast(r.contents.data, C.POINTER(C.c_uint8)), (len(body),))
    assert got.tobytes() == body
    res["inflate"] = {k: stats(v) for k, v in legs.items()}
    res["inflate"]["kernel_inflated_GBps"] = len(body) / (np.median(legs["kernels_ms"]) * 1e-3) / 1e9
    res["inflate"]["upload_GBps"] = len(comp) / (np.median(legs["upload_ms"]) * 1e-3) / 1e9
    res["inflate"]["download_GBps"] = len(body) / (np.median(legs["download_ms"]) * 1e-3) / 1e9
    # ---- the two roads to a read set
    ref = R["ref"]
    o = _lib.BamScanOpts()
    L.lfq_bam_scan_opts_init(C.byref(o))
    rc_ = _lib.BamRecords()
    rc_.n_reads = N_READS
    n_cig, l_seq, l_name = np.ones(N_READS, np.uint32), np.full(N_READS, rb.RL, np.int32), np.full(N_READS, rb.L_QNAME, np.uint16)
    for k, v in (("data", R["data"]), ("data_off", R["data_off"]), ("pos", R["pos"]), ("flag", R["flag"]), ("mapq", R["mapq"]),
                 ("l_qname", l_name), ("n_cigar", n_cig), ("l_qseq", l_seq)):
        setattr(rc_, k, v.ctypes.data)
    rc_.ref = C.cast(C.c_char_p(ref), C.c_void_p)
    rc_.ref_len = len(ref)
    walls = {"from_bgzf": [], "from_bam": []}
    seen = {}
    for p in range(REPS + 1):
        for road in ("from_bgzf", "from_bam"):
            h = C.c_void_p()
            t0 = time.perf_counter()
            if road == "from_bgzf":
                rc = L.lfq_readset_create_from_bgzf(cl.h, comp.ctypes.data, len(comp), 0, -1, C.byref(o),
                                                    C.cast(C.c_char_p(ref), C.c_void_p), len(ref), 0, C.byref(h), None)
            else:
                rc = L.lfq_readset_create_from_bam(cl.h, C.byref(rc_), C.byref(h))
            wall = (time.perf_counter() - t0) * 1e3
            assert rc == 0
            if p:
                walls[road].append(wall)
            seen[road] = {"bgzf": la.last_bgzf_times(cl), "decode": la.last_bam_decode_times(cl)}
            L.lfq_readset_destroy(h)
    res["roads"] = {
        "from_bgzf": {"wall_ms": stats(walls["from_bgzf"]), "link_bytes_down": len(comp),
                      "n_decodes_from_device": seen["from_bgzf"]["bgzf"]["n_decodes_from_device"],
                      "inflate_legs_ms": {k: seen["from_bgzf"]["bgzf"][k] for k in ("upload_ms", "kernels_ms", "download_ms")},
                      "decode_legs_ms": {k: seen["from_bgzf"]["decode"][k] for k in ("upload_ms", "kernels_ms", "download_ms")}},
        "from_bam": {"wall_ms": stats(walls["from_bam"]), "link_bytes_down": int(seen["from_bam"]["decode"]["n_data_bytes"]),
                     "n_decodes_from_device": 0,
                     "decode_legs_ms": {k: seen["from_bam"]["decode"][k] for k in ("upload_ms", "kernels_ms", "download_ms")}}}
    # ---- zlib on the host
    def inflate_all(threads):
        t0 = time.perf_counter()
        if threads == 1:
            n = sum(len(zlib.decompress(x, -15)) for x in raws)
        else:
            with ThreadPoolExecutor(threads) as ex:
                n = sum(ex.map(lambda x: len(zlib.decompress(x, -15)), raws, chunksize=16))
        assert n == len(body)
        return (time.perf_counter() - t0) * 1e3
    res["host_zlib"] = {}
    for th in (1, THREADS):
        v = [inflate_all(th) for _ in range(REPS + 1)][1:]
        res["host_zlib"]["%d_threads" % th] = dict(stats(v), inflated_GBps=len(body) / (np.median(v) * 1e-3) / 1e9)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps({k: res[k] for k in ("inflate", "roads", "host_zlib")}, indent=1))


if __name__ == "__main__":
    main()
