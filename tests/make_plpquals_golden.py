#!/usr/bin/env python
"""Generate tests/golden/plpquals_indel.json, plpquals_srcq.json and plpquals_deep.json from the reference's own 2.1.4 binary
(`make -C oracle ref` unpacks it to oracle/_ref): the COMPLETE stdout of `lofreq plpsummary` (plp_summary, lofreq_call.c:438-599:
header line, the BQ / BAQ / MQ / SQ lines of every nucleotide, the indel lines, the empty line) with the reads as the binary saw
them.  Not a pytest file; data only goes into the fixtures.

  plpquals_indel  reads with insertions, deletions, planted SNVs, BI / BD, a MAPQ mix incl. 0 and 255, run through `lofreq alnqual`
                  first (as oracle/make_golden.py::run_plpindel does) so that the AQ lines carry values; `lofreq plpsummary -f`
  plpquals_srcq   the same kind of reads through `lofreq plpsummary -s -f`: SQ lines, with 49314 in a nucleotide line and in an
                  event line, and a 0 (asserted here)
  plpquals_deep   140 reads of at most 12 bases over 24 bp: a column at least 129 deep with a nucleotide group of more than 64
                  values -- the binary is the witness across the 64 / 128 round boundaries of lfq_plp_group_kernel

All three go through alnqual; the fixtures hold the reads with the lb / ai / ad tags it wrote.  Each stays below 120 KiB (the cap
oracle/make_golden.py::run_baq_edges uses): 40 reads of 90 bases over 120 bp give about 94 KB of text, so the read counts are small.

2.1.4 against the HEAD sources, for these lines: the same format and the same values (compile_plp_col differs in ref_base for
contig letters outside ACGTN only; the contigs here hold A, C, G, T).  Every field is comparable.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
from make_golden import LOFREQ, write_indel_fixture      # noqa: E402

OUT = os.path.join(HERE, "golden")
MAX_BYTES = 120 * 1024


def alnqual_and_summary(tmp, extra):
    """t.sam -> (the reads `lofreq alnqual` wrote, the stdout of `lofreq plpsummary [extra] -f t.fa` on them)"""
    subprocess.check_call([LOFREQ, "faidx", "t.fa"], cwd=tmp)
    with open(os.path.join(tmp, "t.aq.bam"), "wb") as f:
        subprocess.check_call([LOFREQ, "alnqual", "-b", "t.sam", "t.fa"], cwd=tmp, stdout=f)
    sam = subprocess.run([LOFREQ, "alnqual", "t.sam", "t.fa"], cwd=tmp, check=True, capture_output=True, text=True).stdout
    text = subprocess.run([LOFREQ, "plpsummary"] + list(extra) + ["-f", "t.fa", "t.aq.bam"], cwd=tmp, check=True,
                          capture_output=True, text=True).stdout
    reads = []
    for line in sam.splitlines():
        if line.startswith("@"):
            continue
        f = line.split("\t")
        tags = {t[:2]: t[5:] for t in f[11:]}
        reads.append([int(f[3]) - 1, int(f[1]), int(f[4]), f[5], f[9], f[10], tags.get("BI"), tags.get("BD"), tags.get("lb"),
                      tags.get("ai"), tags.get("ad")])
    return reads, text


def store(name, params, extra, genome, reads, text):
    fix = {"name": name, "generator": "tests/make_plpquals_golden.py", "reference_binary": "lofreq 2.1.4 (dist tgz)",
           "command": "lofreq alnqual -b t.sam t.fa > t.aq.bam; lofreq plpsummary %s-f t.fa t.aq.bam" % "".join(a + " " for a in extra),
           "args": list(extra), "params": params, "chrom": "chr1", "genome": genome,
           "read_fields": "pos0, flag, mapq, cigar, seq, qual, BI, BD, lb, ai, ad", "reads": reads,
           "not_comparable": [], "text": text}
    out = json.dumps(fix, separators=(",", ":"))
    assert len(out) < MAX_BYTES, (name, len(out))
    open(os.path.join(OUT, name + ".json"), "w").write(out)
    print("%s: %d reads, %d lines of text (%d bytes), %d bytes" % (name, len(reads), text.count("\n"), len(text), len(out)))


def values(text, what):
    """-> [(line head, [values])] of the lines whose title is `what`"""
    out = []
    for line in text.split("\n"):
        f = line.split("\t")
        if line.startswith("  ") and len(f) == 3 and f[1] == what + " =":
            out.append((f[0].strip(), [int(v) for v in f[2].split()]))
    return out


def write_deep(tmp, seed, glen=24, nreads=140, rl=12):
    """short reads piled on one spot: all of them cover [8, 12); a third of the bases at position 10 are planted, a few reads carry
    a 1-base insertion or deletion after position 9"""
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), glen))
    open(os.path.join(tmp, "t.fa"), "w").write(">chr1\n" + genome + "\n")
    reads = []
    for _ in range(nreads):
        pos = int(rng.integers(0, 9))
        kind = rng.random()
        if kind < 0.06 and pos <= 6:                     # insertion after position 9
            a = 10 - pos
            seq = list(genome[pos:pos + a]) + [str(rng.choice(list("ACGT")))] + list(genome[pos + a:pos + rl - 1])
            cigar = "%dM1I%dM" % (a, rl - 1 - a)
        elif kind < 0.12 and pos <= 6:                   # deletion of position 10
            a = 10 - pos
            seq = list(genome[pos:pos + a]) + list(genome[pos + a + 1:pos + rl + 1])
            cigar = "%dM1D%dM" % (a, rl - a)
        else:
            seq = list(genome[pos:pos + rl])
            cigar = "%dM" % rl
            r = rng.random()
            if r < 0.35:
                seq[10 - pos] = "ACGT"[("ACGT".index(genome[10]) + 1 + int(rng.integers(0, 3))) % 4]
            elif r < 0.38:
                seq[10 - pos] = "N"
        n = len(seq)
        qual = "".join(chr(33 + int(q)) for q in np.clip(np.round(rng.normal(33, 6, n)), 2, 41))
        bi = "".join(chr(33 + int(q)) for q in rng.integers(25, 50, n))
        bd = "".join(chr(33 + int(q)) for q in rng.integers(25, 50, n))
        flag = 16 if rng.random() < 0.5 else 0
        reads.append((pos, flag, int(rng.choice([60, 60, 60, 40, 20, 0, 255])), cigar, "".join(seq), qual, bi, bd))
    reads.sort(key=lambda r: r[0])
    with open(os.path.join(tmp, "t.sam"), "w") as f:
        f.write("@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:chr1\tLN:%d\n" % glen)
        for i, (pos, flag, mapq, cg, sq, q, bi, bd) in enumerate(reads):
            f.write("r%d\t%d\tchr1\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\tBI:Z:%s\tBD:Z:%s\n" % (i, flag, pos + 1, mapq, cg, sq, q, bi, bd))
    return genome


def main():
    mq_mix = [60] * 24 + [40, 30, 20, 10, 0, 255]
    sites = {30: [("+", "AC", 0.5)], 45: [("-", 3, 0.5)], 60: [("+", "G", 0.3), ("+", "GGT", 0.3)],
             75: [("-", 1, 0.4), ("+", "T", 0.2)], 88: [("+", "A", 0.15)]}
    snvs = {30: ("A", 0.3), 31: ("C", 0.3), 50: ("G", 0.3), 75: ("T", 0.4), 90: ("C", 0.35)}
    with tempfile.TemporaryDirectory() as tmp:
        params = {"seed": 101, "glen": 118, "nreads": 30, "sites": {str(k): v for k, v in sites.items()},
                  "planted_snvs": {str(k): v for k, v in snvs.items()}, "mapqs": mq_mix}
        genome, _ = write_indel_fixture(tmp, 101, 118, 30, sites, mq_mix, planted_snvs=snvs)
        reads, text = alnqual_and_summary(tmp, [])
        assert any(v != -1 for _, vals in values(text, "AQ") for v in vals)
        assert any(h in ("+0", "-0") for h, _ in values(text, "IDQ"))
        store("plpquals_indel", params, [], genome, reads, text)
    with tempfile.TemporaryDirectory() as tmp:
        params = {"seed": 103, "glen": 118, "nreads": 26, "sites": {str(k): v for k, v in sites.items()},
                  "planted_snvs": {str(k): v for k, v in snvs.items()}, "mapqs": mq_mix}
        genome, _ = write_indel_fixture(tmp, 103, 118, 26, sites, mq_mix, planted_snvs=snvs)
        reads, text = alnqual_and_summary(tmp, ["-s"])
        sq = values(text, "SQ")
        assert any(49314 in vals for h, vals in sq if h in "ACGTN"), "no 49314 in a nucleotide line"
        assert any(49314 in vals for h, vals in sq if h[0] in "+-"), "no 49314 in an event line"
        assert any(0 in vals for _, vals in sq), "no SQ of 0"
        store("plpquals_srcq", params, ["-s"], genome, reads, text)
    with tempfile.TemporaryDirectory() as tmp:
        params = {"seed": 105, "glen": 24, "nreads": 140, "read_length": 12}
        genome = write_deep(tmp, 105)
        reads, text = alnqual_and_summary(tmp, [])
        assert len(reads) >= 130 and all(len(r[4]) <= 12 for r in reads) and len(genome) <= 24
        groups = [len(vals) for h, vals in values(text, "BQ") if h in "ACGTN"]
        assert max(groups) > 64, max(groups)
        store("plpquals_deep", params, [], genome, reads, text)


if __name__ == "__main__":
    main()
