"""Fixture for lfq_readset_create_from_bam_tags / lfq_readset_baq_fill / lfq_region_set_reuse_tags (tests/golden/tag_reuse.json)
from the reference's own 2.1.4 binary (`make -C oracle ref` -> oracle/_ref/bin/lofreq): a BAM whose reads carry FOREIGN lb / ai / ad
strings -- constant bytes no HMM would write, every subset of the three on every CIGAR shape (M only, insertion, deletion, both),
some strings longer than l_qseq -- beside plain copies of the same reads, so that there are SNV and indel calls.  Stored:

  reads            [pos0, flag, mapq, cigar, letters, qual, {tag: [byte, extra length]}]; tag_reuse_model.fixture_records makes
                   the records of them exactly as they are made here (every read also carries constant BI / BD strings)
  alnqual          the first lb / ai / ad field of every record after `lofreq alnqual` (no -r: extended BAQ, IDAQ on -- the option
                   set of `lofreq call`'s default, lofreq_alnqual.c:76-78), null = no such field
  alnqual_r        the same after `lofreq alnqual -r`: everything recomputed
  vcf / vcf_D / vcf_stripped   the lines of `lofreq call --call-indels --no-default-filter` on the BAM as it is, with -D, and on
                   the BAM without the lb / ai / ad fields -- pairwise different, or the fixture could not tell the modes apart
Data only.  The BAM is written with the standard library (tests/make_bamwrite_golden.py).

    python tests/make_tagreuse_golden.py          (LFQ_GOLDEN_OUT: another output directory)
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_bamwrite_golden as mb  # noqa: E402
import tag_reuse_model as trm  # noqa: E402

LOFREQ = mb.LOFREQ
OUT = os.environ.get("LFQ_GOLDEN_OUT") or os.path.join(HERE, "golden")
SEED = 20262
CALL_ARGS = ["--call-indels", "--no-default-filter"]
P_INS, P_DEL, DEL_LEN = 120, 250, 2         # an inserted base behind P_INS - 1, two deleted bases from P_DEL on
SNVS = {100: "A", 141: "C", 231: "G", 272: "T"}
FOREIGN = {"lb": 35, "ai": 36, "ad": 37}    # '#', '$', '%': qualities 2, 3, 4 throughout


def make_genome(rng):
    g = list(rng.choice(list("ACGT"), 400))
    for at, rep in ((40, "AT" * 8), (114, "CCA" + "T" * 6 + "GAC"), (180, "CAG" * 6), (246, "GTCA" + "AG" * 5), (320, "A" * 9)):
        g[at:at + len(rep)] = rep
    for p, alt in SNVS.items():
        if g[p] == alt:
            g[p] = "ACGT"[("ACGT".index(alt) + 1) % 4]
    return "".join(g)


def make_read(rng, genome, shape, start):
    if shape == "m":
        ops = [("M", 60)]
    elif shape == "i":
        ops = [("M", P_INS - start), ("I", 1), ("M", 59 - (P_INS - start))]
    elif shape == "d":
        ops = [("M", P_DEL - start), ("D", DEL_LEN), ("M", 60 - (P_DEL - start))]
    else:
        ops = [("M", P_INS - start), ("I", 1), ("M", P_DEL - P_INS), ("D", DEL_LEN), ("M", 25)]
    seq, x = [], start
    alt = rng.random() < 0.5                # a read shows the alternate allele at every SNV site it covers, or at none
    for op, ln in ops:
        if op == "M":
            for k in range(ln):
                seq.append(SNVS[x + k] if alt and x + k in SNVS else genome[x + k])
            x += ln
        elif op == "I":
            seq.append("G")
        else:
            x += ln
    return {"pos0": start, "cigar": "".join("%d%s" % (ln, op) for op, ln in ops), "letters": "".join(seq),
            "qual": "".join(chr(33 + int(q)) for q in rng.integers(24, 41, len(seq)))}


def make_reads(rng, genome):
    reads = []
    for si, shape in enumerate("midb"):
        for subset in range(8):
            for k in range(2):
                if shape == "m":
                    start = int(rng.integers(60, 240))
                elif shape == "i":
                    start = P_INS - int(rng.integers(15, 45))
                elif shape == "d":
                    start = P_DEL - int(rng.integers(15, 45))
                else:
                    start = P_INS - int(rng.integers(8, 22))
                r = make_read(rng, genome, shape, start)
                tags = {t: [FOREIGN[t], 3 * k] for b, t in enumerate(("lb", "ai", "ad")) if subset >> b & 1}   # k = 1: longer than l_qseq
                flag, mapq = (16 if (si + subset + k) % 2 else 0), int(rng.choice([60, 60, 60, 40, 30]))
                reads.append([r["pos0"], flag, mapq, r["cigar"], r["letters"], r["qual"], tags])
                reads.append([r["pos0"], flag ^ 16, mapq, r["cigar"], r["letters"], r["qual"], {}])              # the plain copy
    reads.sort(key=lambda r: r[0])
    return reads


def first_fields(parsed):
    out = []
    for r in parsed:
        aux = r["data"][r["l_qname"] + 4 * r["n_cigar"] + (r["l_qseq"] + 1) // 2 + r["l_qseq"]:]
        ff = trm.first_fields(aux)
        row = []
        for t in trm.TAGS:
            if t in ff:
                assert ff[t][0] == "Z"
                row.append(ff[t][1].decode())
            else:
                row.append(None)
        out.append(row)
    return out


def call(tmp, bam, extra, tag):
    env = dict(os.environ)
    env["PATH"] = os.path.dirname(os.path.abspath(LOFREQ)) + ":" + env["PATH"]
    res = subprocess.run([LOFREQ, "call", "-f", "t.fa", "-o", "out_%s.vcf" % tag] + CALL_ARGS + extra + [bam], cwd=tmp, check=True,
                         capture_output=True, text=True, env=env)
    nt = {}
    for line in res.stderr.splitlines():
        if "tests performed" in line:
            nt["indel" if "indel" in line else "snv"] = int(line.split(":")[-1])
    vcf = [l for l in open(os.path.join(tmp, "out_%s.vcf" % tag)).read().splitlines() if not l.startswith("#")]
    return {"vcf": vcf, "num_tests": nt}


def main():
    rng = np.random.default_rng(SEED)
    genome = make_genome(rng)
    fix = {"name": "tag_reuse", "generator": "tests/make_tagreuse_golden.py", "reference_binary": "lofreq 2.1.4 (dist tgz)", "seed": SEED,
           "call_args": CALL_ARGS, "genome": genome, "read_fields": "pos0, flag, mapq, cigar, seq, qual, {tag: [byte, extra length]}",
           "reads": make_reads(rng, genome)}
    reads, recs = trm.fixture_records(fix)
    _, stripped = trm.fixture_records(fix, strip=True)
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.fa"), "w").write(">chr1\n" + genome + "\n")
        subprocess.check_call([LOFREQ, "faidx", "t.fa"], cwd=tmp)
        mb.write_bam(os.path.join(tmp, "in.bam"), genome, recs)
        mb.write_bam(os.path.join(tmp, "stripped.bam"), genome, stripped)
        assert [r["name"] for r in mb.parse_bam(os.path.join(tmp, "in.bam"))] == [r["name"] for r in reads]
        for name, opts in (("alnqual", []), ("alnqual_r", ["-r"])):
            out = mb.run(tmp, [("alnqual", opts)], "in.bam", name)
            assert [r["name"] for r in out] == [r["name"] for r in reads]
            fix[name] = first_fields(out)
        fix["vcf"] = call(tmp, "in.bam", [], "asis")
        fix["vcf_D"] = call(tmp, "in.bam", ["-D"], "D")
        fix["vcf_stripped"] = call(tmp, "stripped.bam", [], "stripped")
    a, b, c = (fix[k]["vcf"] for k in ("vcf", "vcf_D", "vcf_stripped"))
    assert a != b and a != c and b != c, "the three VCFs do not tell the modes apart"
    assert any("INDEL" in l for l in a) and any("INDEL" not in l for l in a)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "tag_reuse.json")
    json.dump(fix, open(path, "w"), separators=(",", ":"))
    print("tag_reuse: %d bytes, %d reads, vcf records %d / %d / %d" % (os.path.getsize(path), len(reads), len(a), len(b), len(c)))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "golden", "bam_write.json"))


if __name__ == "__main__":
    main()
