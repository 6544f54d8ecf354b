"""The .tbi of a dbSNP-shaped .vcf.gz on the device, and a 10 kb region opened through it against the whole-file open (DESIGN.md section 8
item 17) -> profiles/tbi_rate.json

  inputs    profiles/vcf_rate.py's file 2: a synthetic, sorted VCF of 1 000 000 records on five names, compressed with bgzf_deflate in
            blocks that end on line boundaries (vcf_write_gz's cuts)
  device    5 passes after a warm-up, medians and ranges: Vcf.index over the deflate result's tables (lfq_last_vcf_index_times: kernels
            and the lists' way back on the device's clock, the finishing pass on the host's); then, from the .vcf.gz and the index as
            they lie on disk, the whole road of a second file both ways -- bgzf_inflate of everything + Vcf.open(tabix) against
            Vcf.open_indexed of chr3:500 000-510 000 -- on the wall clock, with the blocks and bytes each inflated
  against   `--binary`, on a CPU box where oracle/_ref/bin/lofreq is: the wall time of `lofreq filter --no-defaults -i x.vcf -o x.vcf.gz`
            less that of `-o x.vcf`, 1 warm-up + 3 runs each: what the binary spends on compressing and indexing together

    python profiles/tbi_rate.py [out.json]            python profiles/tbi_rate.py --binary
"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

import vcf_rate  # noqa: E402

PASSES = 5
REGION = (b"chr3", 500_000, 510_000)


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def device_side(la, cl, text):
    import numpy as np
    t0 = time.perf_counter()
    gz, tbi_file = la.vcf_write_gz(cl, text)
    write_ms = (time.perf_counter() - t0) * 1e3
    v = la.Vcf.open(cl, text, tabix=True)
    starts = v.records()["line_start"]
    cuts = la.bam_record_cuts(np.append(starts[:-1], len(text)))
    comp, comp_off, data_off, _ = la.bgzf_deflate(cl, text, cuts=cuts, eof=True)
    assert comp.tobytes() == gz
    runs = []
    for p in range(PASSES + 1):
        t0 = time.perf_counter()
        idx = v.index(data_off, comp_off)
        wall = (time.perf_counter() - t0) * 1e3
        t = la.last_vcf_index_times(cl)
        t["index_wall_ms"] = wall
        idx.close()
        if p:
            runs.append(t)
    v.close()
    res = {k: runs[0][k] for k in ("n_records", "n_chunks", "n_intervals", "n_launches")}
    res.update(text_bytes=len(text), gz_bytes=len(gz), tbi_file_bytes=len(tbi_file), n_blocks=len(data_off) - 1, write_gz_wall_ms_once=round(write_ms, 3))
    for k in ("kernels_ms", "download_ms", "host_ms", "index_wall_ms"):
        res[k] = stats([r[k] for r in runs])
    whole, part = [], []
    for p in range(PASSES + 1):
        t0 = time.perf_counter()
        view = la.bgzf_inflate_view(cl, gz)
        w = la.Vcf.open(cl, view.data, tabix=True)
        t1 = time.perf_counter()
        wb = la.last_bgzf_times(cl)
        n_whole = w.n_records
        w.close()
        t2 = time.perf_counter()
        idx = la.VcfIndex.from_file_bytes(cl, tbi_file)
        t3 = time.perf_counter()
        r = la.Vcf.open_indexed(cl, gz, idx, *REGION)
        t4 = time.perf_counter()
        rb = la.last_bgzf_times(cl)
        n_part = r.n_records
        r.close()
        idx.close()
        if p:
            whole.append((t1 - t0) * 1e3)
            part.append(((t3 - t2) * 1e3, (t4 - t3) * 1e3))
    res["whole_file"] = {"inflate_and_open_wall_ms": stats(whole), "blocks": wb["n_blocks"], "bytes_inflated": wb["n_out_bytes"], "records": n_whole}
    res["region"] = {"name": REGION[0].decode(), "beg": REGION[1], "end": REGION[2], "read_index_wall_ms": stats([a for a, _ in part]),
                     "open_indexed_wall_ms": stats([b for _, b in part]), "blocks": rb["n_blocks"], "bytes_inflated": rb["n_out_bytes"],
                     "records": n_part}
    return res


def binary_side(text):
    exe = os.path.join(ROOT, "oracle", "_ref", "bin", "lofreq")
    if not os.path.exists(exe):
        return "NOT MEASURED: oracle/_ref/bin/lofreq is not there"
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "x.vcf"), "wb").write(text)
        ms = {"o.vcf": [], "o.vcf.gz": []}
        for p in range(4):
            for out in ms:
                for f in (out, out + ".tbi"):
                    if os.path.exists(os.path.join(tmp, f)):
                        os.remove(os.path.join(tmp, f))
                t0 = time.perf_counter()
                r = subprocess.run([exe, "filter", "--no-defaults", "-i", "x.vcf", "-o", out], cwd=tmp, capture_output=True)
                if r.returncode != 0:
                    return "NOT MEASURED: " + r.stderr.decode("latin-1")[-200:]
                if p:
                    ms[out].append((time.perf_counter() - t0) * 1e3)
        plain, gz = stats(ms["o.vcf"]), stats(ms["o.vcf.gz"])
        return {"filter_to_vcf_wall_ms": plain, "filter_to_vcf_gz_and_tbi_wall_ms": gz,
                "compress_and_index_wall_ms": round(gz["median"] - plain["median"], 1), "where": "CPU box, one core"}


def main():
    _one, text = vcf_rate.files()
    if "--binary" in sys.argv:
        print(json.dumps({"binary": binary_side(text)}))
        return
    import lofreq_amd as la
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tbi_rate.json")
    cl = la.SnvCaller(0)
    out = {"passes": PASSES, "device": device_side(la, cl, text)}
    json.dump(out, open(out_path, "w"))
    print(json.dumps(out))
    cl.close()


if __name__ == "__main__":
    main()
