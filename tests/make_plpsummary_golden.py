#!/usr/bin/env python
"""Generate tests/golden/plpsummary_snv.json and plpsummary_indel.json from the reference's own 2.1.4 binary (`make -C oracle
ref` unpacks it to oracle/_ref): the RAW header lines of `lofreq plpsummary` (plp_summary, lofreq_call.c:445-459) for two seeded
read sets, with the reads as the binary saw them.  Not a pytest file; data only goes into the fixtures.

  plpsummary_snv    all-M reads over 400 bp with planted variants; a few bases are turned into N after the generator wrote the
                    SAM (oracle/make_golden.py::write_fixture plants none)
  plpsummary_indel  reads with insertions / deletions and BI / BD tags, including sites where the indel is the consensus

Both stay below 120 KiB (the cap oracle/make_golden.py::run_baq_edges uses), which bounds the depth: about 80x and 55x.

2.1.4 against the HEAD sources, for the fields of the header line: compile_plp_col differs in ref_base only -- HEAD prints 'N' for
a contig letter outside ACGTN (plp.c:819-823), 2.1.4 prints the letter.  The contigs here hold A, C, G, T, where both agree; every
field is comparable.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
from make_golden import LOFREQ, write_fixture, write_indel_fixture      # noqa: E402

OUT = os.path.join(HERE, "golden")
MAX_BYTES = 120 * 1024


def header_lines(tmp, sam):
    subprocess.check_call([LOFREQ, "faidx", "t.fa"], cwd=tmp)
    text = subprocess.run([LOFREQ, "plpsummary", "-f", "t.fa", sam], cwd=tmp, check=True, capture_output=True, text=True).stdout
    return [l + "\n" for l in text.split("\n") if l and not l.startswith(" ")]


def sam_reads(tmp, sam="t.sam"):
    """pos0, flag, mapq, cigar, seq, qual, BI, BD (None where the read has no such tag)"""
    out = []
    for line in open(os.path.join(tmp, sam)):
        if line.startswith("@"):
            continue
        f = line.rstrip("\n").split("\t")
        tags = {t[:2]: t[5:] for t in f[11:]}
        out.append([int(f[3]) - 1, int(f[1]), int(f[4]), f[5], f[9], f[10], tags.get("BI"), tags.get("BD")])
    return out


def plant_n(tmp, seed, n_bases):
    """turn n_bases read bases of t.sam into N, seeded"""
    rng = np.random.default_rng(seed)
    path = os.path.join(tmp, "t.sam")
    lines = open(path).read().split("\n")
    idx = [i for i, l in enumerate(lines) if l and not l.startswith("@")]
    for _ in range(n_bases):
        i = idx[int(rng.integers(0, len(idx)))]
        f = lines[i].split("\t")
        j = int(rng.integers(0, len(f[9])))
        f[9] = f[9][:j] + "N" + f[9][j + 1:]
        lines[i] = "\t".join(f)
    open(path, "w").write("\n".join(lines))


def store(name, params, genome, reads, lines):
    fix = {"name": name, "generator": "tests/make_plpsummary_golden.py", "reference_binary": "lofreq 2.1.4 (dist tgz)",
           "command": "lofreq plpsummary -f t.fa t.sam", "params": params, "chrom": "chr1", "genome": genome,
           "read_fields": "pos0, flag, mapq, cigar, seq, qual, BI, BD", "reads": reads,
           "not_comparable": [], "lines": lines}
    text = json.dumps(fix, separators=(",", ":"))
    assert len(text) < MAX_BYTES, (name, len(text))
    open(os.path.join(OUT, name + ".json"), "w").write(text)
    print("%s: %d reads, %d lines, %d bytes" % (name, len(reads), len(lines), len(text)))


def main():
    mq_mix = [60] * 24 + [40, 30, 20, 10, 0, 255]
    with tempfile.TemporaryDirectory() as tmp:
        planted = {50: ("A", 0.3), 120: ("G", 0.08), 121: ("T", 0.05), 200: [("C", 0.5), ("T", 0.45)], 260: ("A", 0.5),
                   333: ("G", 0.9)}
        params = {"seed": 91, "glen": 400, "nreads": 330, "planted": {str(k): v for k, v in planted.items()}, "mapqs": mq_mix,
                  "n_seed": 92, "n_bases": 40}
        genome = write_fixture(tmp, 91, 400, 330, planted, mq_mix)
        plant_n(tmp, 92, 40)
        store("plpsummary_snv", params, genome, sam_reads(tmp), header_lines(tmp, "t.sam"))
    with tempfile.TemporaryDirectory() as tmp:
        sites = {70: [("+", "AC", 0.85)], 100: [("-", 3, 0.9)], 130: [("+", "G", 0.2), ("+", "GGT", 0.25)],
                 160: [("-", 1, 0.55), ("+", "T", 0.1)], 190: [("+", "A", 0.5)], 230: [("+", "G", 0.6)],
                 250: [("-", 5, 0.3), ("+", "CCCC", 0.05)]}
        snvs = {70: ("A", 0.3), 71: ("C", 0.3), 100: ("G", 0.3), 160: ("T", 0.4), 230: ("C", 0.35), 280: ("A", 0.2)}
        params = {"seed": 93, "glen": 330, "nreads": 200, "sites": {str(k): v for k, v in sites.items()},
                  "planted_snvs": {str(k): v for k, v in snvs.items()}, "mapqs": mq_mix}
        genome, _ = write_indel_fixture(tmp, 93, 330, 200, sites, mq_mix, planted_snvs=snvs)
        store("plpsummary_indel", params, genome, sam_reads(tmp), header_lines(tmp, "t.sam"))


if __name__ == "__main__":
    main()
