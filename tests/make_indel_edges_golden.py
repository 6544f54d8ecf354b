"""Fixture for the gates of the indel caller (tests/golden/indel_edges.json) from the reference's own 2.1.4 binary, which
`make -C oracle ref` unpacks to oracle/_ref/bin/lofreq.  Data only.

  reads   the `reads` rows of the groups gates and poly-AT of tests/indel_edges.py, one behind the other on one contig
          (indel_edges.golden_contig): every read carries its BI / BD indel qualities and the lb / ai / ad tags, so the binary
          computes no alignment quality of its own.  The reads are not stored: the table builds them.
  call    `lofreq call --call-indels --only-indels --no-default-filter -b 1 -a 1 -C 10`: a fixed factor of 1 and sig = 1, so that
          every test whose p-value is below 1 writes a line; min_cov = 10 as in the table.
  stored  the VCF lines, the number of indel tests, per row its span on the contig, the SHA-256 of the SAM text.

    python tests/make_indel_edges_golden.py          (LFQ_GOLDEN_OUT: another output directory)
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import indel_edges as ie  # noqa: E402

OUT = os.environ.get("LFQ_GOLDEN_OUT") or os.path.join(HERE, "golden")
CALL_ARGS = ["--call-indels", "--only-indels", "--no-default-filter", "-b", "1", "-a", "1", "-C", str(ie.MIN_COV)]


def sam_text(ref, reads):
    z = lambda a: bytes(bytearray(a)).decode("latin-1")
    lines = ["@HD\tVN:1.0\tSO:coordinate", "@SQ\tSN:chr1\tLN:%d" % len(ref)]
    for i, r in enumerate(reads):
        f = ["r%d" % i, str(16 if r["reverse"] else 0), "chr1", str(r["pos0"] + 1), str(r["mapq"]),
             "".join("%d%s" % (l, o) for o, l in r["cigar"]), "*", "0", "0", "".join("ACGTN"[c] for c in r["seq"]),
             z(r["qual"] + 33)]
        for tag, key in (("BI", "bi"), ("BD", "bd"), ("lb", "lb"), ("ai", "ai"), ("ad", "ad")):
            assert r[key] is not None, "a read without %s: the binary would compute it" % tag
            f.append("%s:Z:%s" % (tag, z(r[key])))
        lines.append("\t".join(f))
    return "\n".join(lines) + "\n"


def main():
    ref, reads, spans = ie.golden_contig()
    sam = sam_text(ref, reads)
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.fa"), "w").write(">chr1\n" + ref + "\n")
        open(os.path.join(tmp, "t.sam"), "w").write(sam)
        subprocess.check_call([mg.LOFREQ, "faidx", "t.fa"], cwd=tmp)
        env = dict(os.environ)
        env["PATH"] = os.path.dirname(os.path.abspath(mg.LOFREQ)) + ":" + env["PATH"]
        res = subprocess.run([mg.LOFREQ, "call", "-f", "t.fa", "-o", "out.vcf"] + CALL_ARGS + ["t.sam"], cwd=tmp, check=True,
                             capture_output=True, text=True, env=env)
        ntests = None
        for line in res.stderr.splitlines():
            if "Number of indel tests performed" in line:
                ntests = int(line.split(":")[-1])
        vcf = [l for l in open(os.path.join(tmp, "out.vcf")).read().splitlines() if not l.startswith("#")]
    assert ntests is not None
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "indel_edges.json")
    json.dump({"name": "indel_edges", "generator": "tests/make_indel_edges_golden.py", "reference_binary": "lofreq 2.1.4 (dist tgz)",
               "call_args": CALL_ARGS, "contig_len": len(ref), "n_reads": len(reads), "sam_sha256": hashlib.sha256(sam.encode()).hexdigest(),
               "rows": [list(s) for s in spans], "num_indel_tests": ntests, "vcf": vcf}, open(path, "w"), separators=(",", ":"))
    print("indel_edges: %d bytes, %d rows, %d reads, %d tests, %d vcf lines" % (os.path.getsize(path), len(spans), len(reads), ntests,
                                                                              len(vcf)))


if __name__ == "__main__":
    main()
