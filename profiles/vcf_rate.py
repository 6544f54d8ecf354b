"""VCF parsing and `vcfset -a complement` on the device against the 2.1.4 binary -> profiles/vcf_rate.json

  inputs    file 2: a synthetic dbSNP-shaped, sorted VCF of 1 000 000 records on five names; file 1: 10 000 records shaped like `lofreq
            call`'s, every second one at a position (and with the alleles) of file 2
  device    Vcf.open of both, vcfset(complement): 5 passes after a warm-up, medians and ranges; scan, parse, match and emit (plan, scan,
            copy) are device events (lfq_last_vcf_times), upload and download the link legs on the host's clock
  against   the reference binary's `vcfset -a complement` over the same files, file 2 as BGZF with the .tbi tests/make_vcf_golden.py
            writes: wall time of the process on one core, 1 warm-up + 3 runs

    python profiles/vcf_rate.py [out.json]
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

N2, N1, PASSES, COPY_CEILING_GBS = 1_000_000, 10_000, 5, 6290.0
HEAD = b"##fileformat=VCFv4.0\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
NAMES = [b"chr1", b"chr2", b"chr3", b"chr4", b"chr5"]


def files():
    per = N2 // len(NAMES)
    two, one = [HEAD], [HEAD]
    for ci, name in enumerate(NAMES):
        for i in range(per):
            pos = 1000 + 37 * i + (i * 7919 + ci) % 29
            two.append(b"%s\t%d\trs%d\t%s\t%s\t.\t.\tRS=%d;VC=SNV;dbSNPBuildID=150\n"
                       % (name, pos, ci * per + i, b"ACGT"[i % 4:i % 4 + 1], b"CGTA"[i % 4:i % 4 + 1], ci * per + i))
    step = N2 // N1
    for j in range(N1):
        k = j * step
        ci, i = divmod(k, per)
        pos = 1000 + 37 * i + (i * 7919 + ci) % 29 + (j % 2)           # every second one a position of file 2 (or one beside it)
        one.append(b"%s\t%d\t.\t%s\t%s\t%d\tPASS\tDP=%d;AF=0.0%d;SB=%d;DP4=%d,%d,%d,%d\n"
                   % (NAMES[ci], pos, b"ACGT"[i % 4:i % 4 + 1], b"CGTA"[i % 4:i % 4 + 1], 40 + j % 200, 1000 + j % 500, 10 + j % 89, j % 40,
                      400, 500, 20 + j % 30, 25))
    return b"".join(one), b"".join(two)


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def device_side(la, cl, one, two):
    runs = []
    for p in range(PASSES + 1):
        t0 = time.perf_counter()
        v2 = la.Vcf.open(cl, two, tabix=True)
        t1 = time.perf_counter()
        a = la.last_vcf_times(cl)
        v1 = la.Vcf.open(cl, one)
        b = la.last_vcf_times(cl)
        t2 = time.perf_counter()
        out = la.vcfset(v1, v2, op="complement")
        t3 = time.perf_counter()
        c = la.last_vcf_times(cl)
        r = {"open2_wall_ms": (t1 - t0) * 1e3, "vcfset_wall_ms": (t3 - t2) * 1e3, "upload2_ms": a["upload_ms"], "scan2_ms": a["scan_ms"],
             "parse2_ms": a["parse_ms"], "launches2": a["n_launches"], "scan1_ms": b["scan_ms"], "parse1_ms": b["parse_ms"],
             "match_ms": c["match_ms"], "emit_ms": c["emit_ms"], "download_ms": c["download_ms"], "set_launches": c["n_set_launches"],
             "n_out": out["n_out"], "text_bytes": len(out["text"]), "records2": v2.n_records, "records1": v1.n_records}
        v1.close()
        v2.close()
        if p:
            runs.append(r)
    r0 = runs[0]
    res = {k: r0[k] for k in ("launches2", "set_launches", "n_out", "text_bytes", "records1", "records2")}
    res.update(bytes1=len(one), bytes2=len(two))
    for k in ("open2_wall_ms", "vcfset_wall_ms", "upload2_ms", "scan2_ms", "parse2_ms", "scan1_ms", "parse1_ms", "match_ms", "emit_ms", "download_ms"):
        res[k] = stats([r[k] for r in runs])
    res["scan2_GBs"] = round(len(two) / res["scan2_ms"]["median"] / 1e6, 1)
    res["scan2_of_copy_ceiling"] = round(res["scan2_GBs"] / COPY_CEILING_GBS, 4)
    res["emit_GBs"] = round(2 * r0["text_bytes"] / res["emit_ms"]["median"] / 1e6, 2)           # bytes read + bytes written
    res["emit_of_copy_ceiling"] = round(res["emit_GBs"] / COPY_CEILING_GBS, 5)
    res["upload2_GBs"] = round(len(two) / res["upload2_ms"]["median"] / 1e6, 1)
    return res


def binary_side(one, two, want_n_out):
    exe = os.path.join(ROOT, "oracle", "_ref", "bin", "lofreq")
    if not os.path.exists(exe):
        return "NOT MEASURED: oracle/_ref/bin/lofreq is not there"
    import make_vcf_golden as mg
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "one.vcf"), "wb").write(one)
        comp = mg.bgzf(two)
        open(os.path.join(tmp, "two.vcf.gz"), "wb").write(comp)
        open(os.path.join(tmp, "two.vcf.gz.tbi"), "wb").write(mg.tbi_of(two, comp))
        ms = []
        for p in range(4):
            out = os.path.join(tmp, "out.vcf")
            if os.path.exists(out):
                os.remove(out)
            t0 = time.perf_counter()
            r = subprocess.run([exe, "vcfset", "-a", "complement", "-1", "one.vcf", "-2", "two.vcf.gz", "-o", "out.vcf"], cwd=tmp,
                               capture_output=True)
            if p:
                ms.append((time.perf_counter() - t0) * 1e3)
            if r.returncode != 0:
                return "NOT MEASURED: the binary did not take the index: " + r.stderr.decode("latin-1")[-200:]
            n_out = sum(1 for ln in open(out, "rb") if not ln.startswith(b"#"))
            if n_out != want_n_out:
                return "NOT MEASURED: the binary wrote %d records through the Python-written index, the device %d" % (n_out, want_n_out)
        return {"vcfset_complement_wall_ms": stats(ms), "n_out": n_out}


def main():
    import lofreq_amd as la
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vcf_rate.json")
    cl = la.SnvCaller(0)
    one, two = files()
    out = {"passes": PASSES, "copy_ceiling_GBs": COPY_CEILING_GBS}
    out["device"] = device_side(la, cl, one, two)
    out["binary"] = binary_side(one, two, out["device"]["n_out"])
    json.dump(out, open(out_path, "w"))
    print(json.dumps(out))
    cl.close()


if __name__ == "__main__":
    main()
