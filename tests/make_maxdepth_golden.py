"""Fixtures for -d / --max-depth (tests/golden/maxdepth_*.json) from the reference's own 2.1.4 binary, which
`make -C oracle ref` unpacks to oracle/_ref/bin/lofreq.  Data only; the prefix keeps them out of the globs of the other
fixture families (golden_util.conf_kwargs does not take -d).

  maxdepth_stacks  hand-placed runs of reads: a run longer than the cap, the first read of a run (always kept), reads that
                   end exactly where a run starts (exclusive end == P still counts), a short first read in front of long
                   ones (positions covered by dropped reads only: no column), S / D / N operations, both strands.  Per cap
                   the plpsummary columns (bases per strand and nucleotide) and the VCF + test count of `lofreq call -d`.
  maxdepth_chain   chain_default-shaped random reads (300 bp, 700 x 100M) at -d 20 and -d 100, with and without
                   --no-default-filter: the VCF and the test count.
  maxdepth_indel   tests/golden_reads.py reads with planted indels and BI / BD tags (3 kb, 150-250x),
                   `--call-indels -d 60`: the VCF and both test counts.
  maxdepth_c4      the big_c4_indels shape (24 kb x 500x, BI / BD) with `--call-indels -d 200`.
  The last two hold the generator's parameters and the SHA-256 of the SAM text, not the reads.

    python tests/make_maxdepth_golden.py          (LFQ_GOLDEN_OUT: another output directory)
"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

OUT = os.environ.get("LFQ_GOLDEN_OUT") or os.path.join(HERE, "golden")
STACK_CAPS = [1, 2, 3, 7, 40, 1000000]
CHAIN_CAPS = [20, 100]


def stacks_reads(seed=7, glen=420):
    """[(pos0, flag, mapq, cigar, seq, qual)] in file order"""
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), glen))
    alt = {110: "T", 160: "G", 250: "C", 330: "A"}          # planted in every other read that covers them
    runs = [  # (pos0, [cigar, ...])
        (99, ["60M"] * 10),                                 # longer than every small cap
        (100, ["60M"] * 4),
        (149, ["10M"] + ["60M"] * 5),                       # short first read: [159, 209) is covered by the later ones only
        (200, ["40M"] * 3),                                 # exclusive end 240 ...
        (240, ["30M"] * 3),                                 # ... still counts at 240
        (241, ["30M"] * 3),                                 # ... and no longer at 241
        (300, ["5S45M", "20M3D25M", "10M40N35M", "45M5S", "15M2I28M", "45M", "45M"]),
    ]
    reads = []
    k = 0
    for pos0, cigars in runs:
        for cg in cigars:
            seq, x, y = [], pos0, 0
            for n, op in [(int(a), b) for a, b in re.findall(r"(\d+)([MIDNS])", cg)]:
                if op == "M":
                    for j in range(n):
                        b = genome[x + j]
                        if x + j in alt and k % 2 == 0:
                            b = alt[x + j]
                        seq.append(b)
                    x += n
                elif op in "IS":
                    seq.extend(rng.choice(list("ACGT"), n))
                elif op in "DN":
                    x += n
            qual = "".join(chr(33 + int(q)) for q in rng.integers(25, 41, len(seq)))
            reads.append((pos0, 16 if k % 3 == 1 else 0, 60, cg, "".join(seq), qual))
            k += 1
    return genome, reads


def write_sam(tmp, genome, reads):
    open(os.path.join(tmp, "t.fa"), "w").write(">chr1\n" + genome + "\n")
    with open(os.path.join(tmp, "t.sam"), "w") as f:
        f.write("@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:chr1\tLN:%d\n" % len(genome))
        for i, (pos0, flag, mapq, cg, seq, q) in enumerate(reads):
            f.write("r%d\t%d\tchr1\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\n" % (i, flag, pos0 + 1, mapq, cg, seq, q))


def call(tmp, args):
    env = dict(os.environ)
    env["PATH"] = os.path.dirname(os.path.abspath(mg.LOFREQ)) + ":" + env["PATH"]
    if os.path.exists(os.path.join(tmp, "out.vcf")):
        os.remove(os.path.join(tmp, "out.vcf"))
    res = subprocess.run([mg.LOFREQ, "call", "-f", "t.fa", "-o", "out.vcf"] + args + ["t.sam"], cwd=tmp, check=True,
                         capture_output=True, text=True, env=env)
    ntests = {}
    for line in res.stderr.splitlines():
        if "tests performed" in line:
            ntests["indel" if "indel" in line else "snv"] = int(line.split(":")[-1])
    vcf = [l for l in open(os.path.join(tmp, "out.vcf")).read().splitlines() if not l.startswith("#")]
    return vcf, ntests


def read_sam(tmp):
    reads = []
    for line in open(os.path.join(tmp, "t.sam")):
        if line.startswith("@"):
            continue
        f = line.rstrip("\n").split("\t")
        reads.append([int(f[3]) - 1, int(f[1]), int(f[4]), f[5], f[9], f[10]])
    return reads


def dump(name, fix):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".json")
    json.dump(fix, open(path, "w"), separators=(",", ":"))
    print("%s: %d bytes" % (name, os.path.getsize(path)))


def main_stacks():
    genome, reads = stacks_reads()
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        write_sam(tmp, genome, reads)
        subprocess.check_call([mg.LOFREQ, "faidx", "t.fa"], cwd=tmp)
        for d in STACK_CAPS:
            plp = subprocess.run([mg.LOFREQ, "plpsummary", "-f", "t.fa", "-d", str(d), "t.sam"], cwd=tmp, check=True,
                                 capture_output=True, text=True).stdout
            cols = [{"pos0": c["pos0"], "fwrv": c["fwrv"]} for c in mg.parse_plpsummary(plp)]
            vcf, ntests = call(tmp, ["-d", str(d)])
            runs.append({"max_depth": d, "call_args": [], "columns": cols, "vcf": vcf, "num_snv_tests": ntests["snv"]})
        stored = read_sam(tmp)
    dump("maxdepth_stacks", {"name": "maxdepth_stacks", "generator": "tests/make_maxdepth_golden.py",
                             "reference_binary": "lofreq 2.1.4 (dist tgz)", "genome": genome, "reads": stored, "runs": runs})


def main_chain():
    mq_mix = [60] * 24 + [40, 30, 20, 10, 0, 255]
    planted = {60: ("A", 0.05), 61: ("C", 0.05), 90: ("C", 0.10), 120: ("G", 0.03), 150: ("T", 0.5), 180: ("C", 1.0),
               200: ("T", 0.07), 230: ("A", 0.02)}
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        genome = mg.write_fixture(tmp, 41, 300, 700, planted, mq_mix, min_q=6)
        subprocess.check_call([mg.LOFREQ, "faidx", "t.fa"], cwd=tmp)
        for d in CHAIN_CAPS:
            for extra in ([], ["--no-default-filter"]):
                vcf, ntests = call(tmp, ["-d", str(d)] + extra)
                runs.append({"max_depth": d, "call_args": extra, "vcf": vcf, "num_snv_tests": ntests["snv"]})
        stored = read_sam(tmp)
    dump("maxdepth_chain", {"name": "maxdepth_chain", "generator": "tests/make_maxdepth_golden.py",
                            "reference_binary": "lofreq 2.1.4 (dist tgz)", "genome": genome, "reads": stored, "runs": runs})


def run_generated(name, params, call_args, max_depth):
    """reads of tests/golden_reads.py -> SAM -> `lofreq call <call_args> -d <max_depth>`; the reads are not stored"""
    import golden_reads as gr
    with tempfile.TemporaryDirectory() as tmp:
        R = gr.make(**params)
        open(os.path.join(tmp, "t.fa"), "w").write(">chr1\n" + R["ref"].decode() + "\n")
        sha = gr.write_sam(R, os.path.join(tmp, "t.sam"))
        subprocess.check_call([mg.LOFREQ, "faidx", "t.fa"], cwd=tmp)
        vcf, ntests = call(tmp, call_args + ["-d", str(max_depth)])
    dump(name, {"name": name, "generator": {"module": "tests/golden_reads.py", "version": gr.GENERATOR_VERSION, "params": params},
                "reference_binary": "lofreq 2.1.4 (dist tgz)", "call_args": call_args, "max_depth": max_depth,
                "n_reads": int(R["n"]), "sam_sha256": sha, "num_tests": ntests, "vcf": vcf})


def main_generated():
    run_generated("maxdepth_indel", dict(seed=611, glen=3000, depth_lo=150, depth_hi=250, min_q=6, snv_every=40,
                                         indel_every=120), ["--call-indels"], 60)
    run_generated("maxdepth_c4", dict(seed=603, glen=24000, depth_lo=500, depth_hi=500, min_q=6, snv_every=60,
                                      indel_every=240), ["--call-indels"], 200)


if __name__ == "__main__":
    main_stacks()
    main_chain()
    main_generated()
