"""Fixtures for `lofreq indelqual` (tests/golden/indelqual_*.json) from the reference's own 2.1.4 binary, which
`make -C oracle ref` unpacks to oracle/_ref/bin/lofreq: seeded reads (tests/indelqual_reads.py) as SAM + FASTA ->
`lofreq indelqual --dindel -f t.fa -o out.bam t.sam` and `lofreq indelqual -u 40 | 40,100 | -5 -o out.bam t.sam` -> the BI and BD
strings of every record of the BAM it writes, run-length encoded (tests/indelqual_model.py: rle).  Data only.

  indelqual_small   a few hundred reads, held inline (contig, reads, results)
  indelqual_shapes  a few thousand, regenerated from the seed: generator parameters and version, SHA-256 of the SAM text, results
  indelqual_e2e     position-sorted reads of tests/golden_reads.py WITHOUT BI / BD -> `indelqual --dindel` ->
                    `call --call-indels --no-default-filter -f t.fa`: the VCF lines and the two test counts; the indel lines the same
                    reads give after `indelqual -u 40`, for the test that the Dindel qualities matter to the calls

The BAM is read with the standard library: BGZF is a series of gzip members; BI / BD are the only aux fields of a record.

    python tests/make_indelqual_golden.py          (LFQ_GOLDEN_OUT: another output directory)
"""
import gzip
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import golden_reads as gr  # noqa: E402
import indelqual_model as im  # noqa: E402
import indelqual_reads as ir  # noqa: E402
import viterbi_reads as vr  # noqa: E402

LOFREQ = os.path.join(ROOT, "oracle", "_ref", "bin", "lofreq")
OUT = os.environ.get("LFQ_GOLDEN_OUT") or os.path.join(HERE, "golden")
SMALL = dict(seed=9101, n=300, glen=1500)
SHAPES = dict(seed=9102, n=2400, glen=3000)
E2E = dict(seed=77, glen=8000, depth_lo=200, depth_hi=400, indel_every=120)
E2E_CALL = ["--call-indels", "--no-default-filter"]


def parse_bam(path):
    """[(name, {tag: string})] of the Z tags of every record"""
    data = gzip.decompress(open(path, "rb").read())
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", data, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, o)
    o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, o)
        o += 4 + l_name + 4
    recs = []
    while o < len(data):
        block_size, _ref_id, _pos, l_name, _mapq, _bin, n_cigar, _flag, l_seq = struct.unpack_from("<iiiBBHHHi", data, o)
        name = data[o + 36:o + 36 + l_name - 1].decode()
        a = o + 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
        end = o + 4 + block_size
        tags = {}
        while a < end:
            tag, typ = data[a:a + 2].decode(), data[a + 2:a + 3]
            assert typ == b"Z", (name, tag, typ)
            z = data.index(b"\0", a + 3)
            tags[tag] = data[a + 3:z].decode()
            a = z + 1
        recs.append((name, tags))
        o = end
    return recs


def run_indelqual(tmp, sam, mode, names):
    out = os.path.join(tmp, "out_%s.bam" % mode.replace(",", "_"))
    subprocess.run([LOFREQ, "indelqual"] + ir.mode_args(mode) + ["-o", out, sam], cwd=tmp, check=True, capture_output=True)
    recs = parse_bam(out)
    assert [n for n, _ in recs] == names, "records out of order or missing"
    assert all(sorted(t) == ["BD", "BI"] for _, t in recs)
    return out, recs


def run_family(genome, reads):
    """-> (sha256 of the SAM text, {mode: what indelqual_reads.fixture_tags reads})"""
    text = vr.sam_text(genome, reads)
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.fa"), "w").write(">chr1\n" + genome + "\n")
        open(os.path.join(tmp, "t.sam"), "w").write(text)
        subprocess.check_call([LOFREQ, "faidx", "t.fa"], cwd=tmp)
        for mode in ir.MODES:
            _, recs = run_indelqual(tmp, "t.sam", mode, [r["name"] for r in reads])
            if mode == "dindel":
                bi = [im.rle(t["BI"]) for _, t in recs]
                bd = [im.rle(t["BD"]) for _, t in recs]
                res[mode] = {"bi": bi, "bd": None if bd == bi else bd}
            else:                                               # one byte per tag, repeated: the byte and every record's length
                bi_byte, bd_byte = recs[0][1]["BI"][0], recs[0][1]["BD"][0]
                assert all(t["BI"] == bi_byte * len(t["BI"]) and t["BD"] == bd_byte * len(t["BI"]) for _, t in recs)
                res[mode] = {"bi_byte": bi_byte, "bd_byte": bd_byte, "len": [len(t["BI"]) for _, t in recs]}
    return vr.sha256(text), res


def run_e2e():
    R = gr.make(**E2E)
    R["bi"] = R["bd"] = None                                    # the tags are what the command under test adds
    names = ["r%d" % i for i in range(R["n"])]
    env = dict(os.environ)
    env["PATH"] = os.path.dirname(os.path.abspath(LOFREQ)) + ":" + env["PATH"]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.fa"), "w").write(">chr1\n" + R["ref"].decode() + "\n")
        sha = gr.write_sam(R, os.path.join(tmp, "t.sam"))
        subprocess.check_call([LOFREQ, "faidx", "t.fa"], cwd=tmp)
        for mode in ("dindel", "u40"):
            t0 = time.time()
            bam, _ = run_indelqual(tmp, "t.sam", mode, names)
            secs = time.time() - t0
            vcf_path = os.path.join(tmp, "out_%s.vcf" % mode)
            res = subprocess.run([LOFREQ, "call", "-f", "t.fa", "-o", vcf_path] + E2E_CALL + [bam], cwd=tmp, check=True,
                                 capture_output=True, text=True, env=env)
            nt = {}
            for line in res.stderr.splitlines():
                if "tests performed" in line:
                    nt["indel" if "indel" in line else "snv"] = int(line.split(":")[-1])
            vcf = [l for l in open(vcf_path).read().splitlines() if not l.startswith("#")]
            out[mode] = (vcf, nt, secs)
    vcf, nt, secs = out["dindel"]
    is_indel = lambda l: "INDEL" in l.split("\t")[7]
    return {"name": "indelqual_e2e", "generator": {"module": "tests/golden_reads.py", "version": gr.GENERATOR_VERSION, "params": E2E,
                                                    "then": "bi = bd = None"},
            "reference_binary": "lofreq 2.1.4 (dist tgz)",
            "command": "lofreq indelqual --dindel -f t.fa -o q.bam t.sam; lofreq call -f t.fa --call-indels --no-default-filter q.bam",
            "call_args": E2E_CALL, "n_reads": int(R["n"]), "sam_sha256": sha, "num_tests": nt, "vcf": vcf,
            "n_indel_lines": sum(1 for l in vcf if is_indel(l)),
            "indel_lines_after_uniform_40": [l for l in out["u40"][0] if is_indel(l)],
            "indelqual_seconds_in_the_build_container": round(secs, 3)}


def dump(name, fix):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".json")
    json.dump(fix, open(path, "w"), separators=(",", ":"))
    print("%s: %d bytes" % (name, os.path.getsize(path)))


def main():
    for name, params, inline in (("indelqual_small", SMALL, True), ("indelqual_shapes", SHAPES, False)):
        R = ir.make(**params)
        sha, res = run_family(R["genome"], R["reads"])
        fix = {"name": name, "generator": {"module": "tests/indelqual_reads.py", "version": ir.GENERATOR_VERSION, "params": params},
               "reference_binary": "lofreq 2.1.4 (dist tgz)",
               "command": "lofreq indelqual (--dindel -f t.fa | -u 40 | -u 40,100 | -u -5) -o out.bam t.sam",
               "n_reads": len(R["reads"]), "sam_sha256": sha, "results": res}
        if inline:
            fix["genome"] = R["genome"]
            fix["reads"] = [[r["name"], r["pos0"], "".join("%d%s" % (l, o) for o, l in r["cigar"]), len(r["seq"])] for r in R["reads"]]
        dump(name, fix)
    dump("indelqual_e2e", run_e2e())


if __name__ == "__main__":
    main()
