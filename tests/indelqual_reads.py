"""Seeded reads for `lofreq indelqual` (tests/golden/indelqual_*.json, tests/test_indelqual_model.py, tests/test_gpu_indelqual.py):
the families of tests/viterbi_reads.py -- M I D S H = X operations, soft clips, reads clipped at either end of the contig -- over
a contig in which homopolymer runs of every length 2 .. 25, runs of N and lower-case runs are planted, so that every letter of
the Dindel table occurs.  Reads with an N / P operation are left out (the command exits on them); one read ending on the contig's
last base and one reaching past it are added."""
import numpy as np

import viterbi_reads as vr

GENERATOR_VERSION = 1
MODES = ("dindel", "u40", "u40,100", "u-5")


def plant_runs(genome, seed):
    rng = np.random.default_rng([GENERATOR_VERSION, seed])
    g = list(genome)
    glen = len(g)
    slots = rng.permutation(np.arange(40, glen - 60, 34))           # non-overlapping places: a run and a guard base behind it
    k = 0
    for rep in range(max(1, glen // 1500)):
        for L in range(2, 26):
            if k >= len(slots):
                break
            s = int(slots[k])
            k += 1
            kind = (L + rep) % 9
            letter = "N" if kind == 0 else "acgt"[L % 4] if kind in (1, 2) else "ACGT"[int(rng.integers(4))]
            g[s:s + L] = letter * L
            for p in (s - 1, s + L):                                # the run is exactly L long
                while g[p].upper() == letter.upper():
                    g[p] = "ACGT"[int(rng.integers(4))]
            if kind == 3:
                g[s + L // 2] = g[s].lower()                        # mixed case inside one run
    g[glen - 7:glen - 3] = "GGGG"                                   # a run right in front of the contig's end
    g[glen - 3:] = "CAT"
    return "".join(g)


def make(seed, n, glen):
    """-> {"genome": str, "reads": [{name, pos0, cigar [(op, len)], seq, qual, shape}]}"""
    R = vr.make(seed=seed, n=n, glen=glen)
    genome = plant_runs(R["genome"], seed)
    reads = [r for r in R["reads"] if not any(o in "NP" for o, _ in r["cigar"])]
    for name, cigar, pos0 in (("end0", [("S", 3), ("M", 40)], glen - 40), ("end1", [("M", 30), ("I", 2), ("M", 10)], glen - 40),
                              ("past", [("M", 36)], glen - 30), ("first", [("M", 20), ("D", 3), ("X", 16)], 0)):
        lq = sum(l for o, l in cigar if o in "MIS=X")
        reads.append({"name": name, "pos0": pos0, "cigar": cigar, "seq": "A" * lq, "qual": [30] * lq, "shape": "edge"})
    return {"genome": genome, "reads": reads}


def mode_args(mode):
    """the command line of a fixture mode"""
    return ["--dindel", "-f", "t.fa"] if mode == "dindel" else ["-u", mode[1:]]


def mode_quals(mode):
    """-> (ins_qual, del_qual) of a uniform mode"""
    v = [int(x) for x in mode[1:].split(",")]
    return v[0], v[-1]


def fixture_tags(res, i):
    """(BI, BD) of read i as the binary wrote them, from a fixture's results[mode]: Dindel strings are run-length encoded
    ("bd": None = the same strings as "bi"), a uniform mode is its two bytes and the length of every record's tags"""
    import indelqual_model as im
    if "bi_byte" in res:
        return res["bi_byte"] * res["len"][i], res["bd_byte"] * res["len"][i]
    bi = im.unrle(res["bi"][i])
    return bi, bi if res["bd"] is None else im.unrle(res["bd"][i])
