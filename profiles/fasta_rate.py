"""`lofreq faidx` and the whole-contig fetch on the device against the 2.1.4 binary and the one-thread host loop (DESIGN.md section 8
item 16) -> profiles/fasta_rate.json

  inputs    one synthetic contig of 250 Mb at width 60; a file of the same size with 3 000 contigs; the big contig again with one
            blank inside every line (equal line bytes, one base fewer: the general fetch path)
  device    Fasta.open, FastaIndex.build and Fasta.fetch of the (first) contig: 5 passes after a warm-up, medians and ranges.  scan,
            lines and fetch are device events (lfq_last_fasta_times), GB/s over the file's bytes (scan, lines) and over the contig's
            (fetch); upload and download are the link legs on the host's clock; wall is the whole call
  against   `lofreq faidx` and `lofreq checkref` of the reference binary (oracle/_ref/bin/lofreq) on the same file, wall time of the
            process, 1 warm-up + 3 runs; lfq_fasta_check --time, the host loop of lfq_fasta.h in one thread

    python profiles/fasta_rate.py [out.json]
"""
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

N, WIDTH, PASSES, COPY_CEILING_GBS = 250_000_000, 60, 5, 6290.0


def contig_lines(n, width, seed, blank=False):
    rng = np.random.default_rng(seed)
    rows = n // width
    a = np.empty((rows, width + 1), np.uint8)
    a[:, :width] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (rows, width), dtype=np.uint8)]
    a[:, width] = 0x0a
    if blank:
        a[np.arange(rows), np.arange(rows) % width] = 0x20
    return a.reshape(-1)


def one_contig(blank=False):
    return np.concatenate([np.frombuffer(b">big\n", np.uint8), contig_lines(N, WIDTH, 1, blank)])


def many_contigs(k=3000):
    per = N // k // WIDTH * WIDTH
    body = contig_lines(per, WIDTH, 2)
    return np.concatenate([x for i in range(k) for x in (np.frombuffer(b">c%d\n" % i, np.uint8), body)])


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def device_side(la, cl, data, name):
    runs = []
    for p in range(PASSES + 1):
        t0 = time.perf_counter()
        fa = la.Fasta.open(cl, data)
        t1 = time.perf_counter()
        idx = la.FastaIndex.build(fa)
        t2 = time.perf_counter()
        ref = fa.fetch(idx, name)
        t3 = time.perf_counter()
        t = la.last_fasta_times(cl)
        t.update(open_wall_ms=(t1 - t0) * 1e3, build_wall_ms=(t2 - t1) * 1e3, fetch_wall_ms=(t3 - t2) * 1e3, contig=len(ref),
                 entries=len(idx.entries))
        fa.close()
        if p:
            runs.append(t)
    r0 = runs[0]
    out = {"file_bytes": int(r0["n_bytes"]), "lines": int(r0["n_lines"]), "headers": int(r0["n_headers"]), "entries": r0["entries"],
           "contig_bases": r0["contig"], "fetch_path": {1: "regular", 2: "general"}[r0["fetch_path"]], "launches": r0["n_launches"]}
    for k in ("upload_ms", "scan_ms", "lines_ms", "fetch_ms", "download_ms", "open_wall_ms", "build_wall_ms", "fetch_wall_ms"):
        out[k] = stats([r[k] for r in runs])
    out["scan_GBs"] = round(r0["n_bytes"] / out["scan_ms"]["median"] / 1e6, 1)
    out["lines_GBs"] = round(r0["n_bytes"] / out["lines_ms"]["median"] / 1e6, 1)
    out["fetch_GBs"] = round(2 * r0["contig"] / out["fetch_ms"]["median"] / 1e6, 1)      # bytes read + bytes written
    out["upload_GBs"] = round(r0["n_bytes"] / out["upload_ms"]["median"] / 1e6, 1)
    out["download_GBs"] = round(r0["contig"] / out["download_ms"]["median"] / 1e6, 1)
    return out


def binary_side(data, names_lens):
    exe = os.path.join(ROOT, "oracle", "_ref", "bin", "lofreq")
    if not os.path.exists(exe):
        return "NOT MEASURED: oracle/_ref/bin/lofreq is not there"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        data.tofile(os.path.join(tmp, "t.fa"))
        with open(os.path.join(tmp, "t.sam"), "w") as f:
            f.write("@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % x for x in names_lens))
        for what, args in (("faidx", ["faidx", "t.fa"]), ("checkref", ["checkref", "t.fa", "t.sam"])):
            ms = []
            for p in range(4):
                if what == "faidx" and os.path.exists(os.path.join(tmp, "t.fa.fai")):
                    os.remove(os.path.join(tmp, "t.fa.fai"))
                t0 = time.perf_counter()
                r = subprocess.run([exe] + args, cwd=tmp, capture_output=True)
                if p:
                    ms.append((time.perf_counter() - t0) * 1e3)
                assert r.returncode == 0, r.stderr[-300:]
            out[what + "_wall_ms"] = stats(ms)
    return out


def host_loop():
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        return "NOT MEASURED: no host compiler"
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "lfq_fasta_check")
        subprocess.check_call([cxx, "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "lofreq_amd", "csrc"),
                               os.path.join(ROOT, "lofreq_amd", "csrc", "lfq_fasta_check.cpp"), "-o", exe])
        runs = [json.loads(subprocess.check_output([exe, "--time", str(N + N // WIDTH)]))["build_ms"] for _ in range(4)][1:]
    return {"build_ms": stats(runs)}


def main():
    import lofreq_amd as la
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fasta_rate.json")
    cl = la.SnvCaller(0)
    out = {"passes": PASSES, "copy_ceiling_GBs": COPY_CEILING_GBS, "width": WIDTH}
    big = one_contig()
    out["one_contig"] = device_side(la, cl, big, "big")
    out["one_contig"]["binary"] = binary_side(big, [("big", out["one_contig"]["contig_bases"])])
    del big
    many = many_contigs()
    out["many_contigs"] = device_side(la, cl, many, "c0")
    del many
    blank = one_contig(blank=True)
    out["one_contig_one_blank_per_line"] = device_side(la, cl, blank, "big")
    del blank
    out["general_over_regular"] = round(out["one_contig_one_blank_per_line"]["fetch_ms"]["median"] / out["one_contig"]["fetch_ms"]["median"], 2)
    out["host_loop_one_thread"] = host_loop()
    json.dump(out, open(out_path, "w"), indent=1)
    print(json.dumps(out))
    cl.close()


if __name__ == "__main__":
    main()
