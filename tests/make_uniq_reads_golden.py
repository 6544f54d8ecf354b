"""tests/golden/uniq_reads.json: `lofreq uniq` of the reference's own 2.1.4 binary (oracle/_ref/bin/lofreq, unpacked by
`make -C oracle ref`) on a small BAM whose READS are stored, for the read-level road (lfq_readset_uniq).  Data only.

  reads     a 600 bp genome, about 300 reads of 30-60 bases: M, soft clips at both ends, I, D, N, one read with 5H; both
            strands; MAPQ 0, 1, 60 and 255; flags with paired / not-proper-pair, secondary, QC-fail and duplicate (the binary
            drops those reads itself; a test applies uniq's filter -- uniq_sites_cases.uniq_filter -- before it creates a read set);
            qualities 2..41 (2 is below min_plp_bq = 3); planted alt bases; two insertions of equal length and different
            sequence at one position; an insertion with an N; deletions of two lengths at one position; a stretch that only
            reads ending at the same base cover, and next to it a position no read covers.
  variants  about 60: SNVs at planted and clean sites, matching and non-matching insertions and deletions, a deletion whose
            REF disagrees with the genome, variants with only the INDEL key, several variants at one position, the uncovered
            position, the all-tails position; AF strings including 0.000000 and 1.000000.
  runs      alnqual -b -> index -> `uniq --output-all`, `uniq --use-det-lim --output-all`, `uniq --uni-freq 0.5 --output-all`;
            per variant and run the UQ= value (null: no tag), the UNIQ flag and the FILTER column.

    python tests/make_uniq_reads_golden.py          (LFQ_GOLDEN_OUT: another output directory)
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
from uniq_sites_cases import uniq_filter  # noqa: E402

OUT = os.environ.get("LFQ_GOLDEN_OUT") or os.path.join(HERE, "golden")
GLEN = 600
INS_POS, INS_N_POS, DEL_POS, TAIL_POS, BARE_POS = 150, 200, 250, 400, 405
HOLE = (TAIL_POS - 12, 412)         # [a, b): only the reads that end at TAIL_POS reach in here, and none gets past TAIL_POS
PLANTED = {60: ("T", 0.5), 90: ("A", 0.2), 120: ("C", 0.08), 300: ("G", 1.0), 330: ("A", 0.03), 500: ("C", 0.3)}
RUNS = {"default": ["--output-all"], "detlim": ["--use-det-lim", "--output-all"], "unifreq": ["--uni-freq", "0.5", "--output-all"]}


def make_reads(seed=2024):
    """-> (genome, [(pos0, flag, mapq, cigar, seq, qual)] sorted by pos0)"""
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), GLEN))
    # `lofreq uniq` gives its mpileup no FASTA (lofreq_uniq.c:459-465 sets no mplp_conf.fa), so the binary's key of EVERY deletion is
    # a run of N (plp.c:1136: no ref -> 'N') whatever the genome holds; the contig carries N under the planted deletions, where
    # a key built from the contig and the binary's agree.  The reads over the stretch carry N bases as well.
    genome = genome[:DEL_POS + 1] + "NNNN" + genome[DEL_POS + 5:]
    other = lambda b: "ACGT"[("ACGT".index(b) + 1 + int(rng.integers(0, 3))) % 4]
    flags = [0, 16] * 10 + [3, 19, 1, 17, 65, 256, 272, 512, 1024, 1040]
    mapqs = [60] * 20 + [0, 1, 1, 255, 255, 30]
    reads = []

    def add(pos0, cigar, ins=None, flag=None, mapq=None):
        seq, x = [], pos0
        for n, op in [(int(a), b) for a, b in re.findall(r"(\d+)([MIDNSH])", cigar)]:
            if op == "M":
                for j in range(n):
                    b = genome[x + j]
                    if x + j in PLANTED and rng.random() < PLANTED[x + j][1]:
                        b = PLANTED[x + j][0]
                    elif b != "N" and rng.random() < 0.01:
                        b = other(b)
                    seq.append(b)
                x += n
            elif op == "I":
                seq.extend(ins if ins is not None else rng.choice(list("ACGT"), n))
            elif op == "S":
                seq.extend(rng.choice(list("ACGT"), n))
            elif op in "DN":
                x += n
        q = rng.integers(20, 42, len(seq))
        q[rng.random(len(seq)) < 0.06] = 2
        q[rng.random(len(seq)) < 0.04] = 3
        reads.append((pos0, int(rng.choice(flags)) if flag is None else flag, int(rng.choice(mapqs)) if mapq is None else mapq,
                      cigar, "".join(seq), "".join(chr(33 + int(v)) for v in q)))

    def free(pos0, span):           # may a read lie at [pos0, pos0 + span)?
        return pos0 + span <= HOLE[0] or pos0 >= HOLE[1]

    n_plain = 0
    while n_plain < 230:
        ln = int(rng.integers(30, 61))
        pos0 = int(rng.integers(0, GLEN - ln))
        if not free(pos0, ln):
            continue
        kind = int(rng.integers(0, 12))
        if kind == 0:
            a = int(rng.integers(1, 6))
            add(pos0, "%dS%dM%dS" % (a, ln - a - 3, 3))
        elif kind == 1 and free(pos0, ln + 3):
            add(pos0, "%dM3D%dM" % (ln // 2, ln - ln // 2))
        elif kind == 2 and free(pos0, ln + 25) and pos0 + ln + 25 < GLEN:
            add(pos0, "%dM25N%dM" % (ln // 3, ln - ln // 3))
        elif kind == 3:
            add(pos0, "%dM2I%dM" % (ln // 2, ln - ln // 2 - 2))
        else:
            add(pos0, "%dM" % ln)
        n_plain += 1
    add(20, "5H30M")
    for k in range(14):             # two insertions of equal length and different sequence at one position
        a = 12 + k
        add(INS_POS + 1 - a, "%dM2I%dM" % (a, 20 + k), ins="AT" if k % 3 else "AC", flag=16 * (k % 2), mapq=60)
    for k in range(6):              # an insertion with an N
        a = 15 + 2 * k
        add(INS_N_POS + 1 - a, "%dM2I%dM" % (a, 22), ins="AN" if k % 2 == 0 else "AA", flag=16 * (k % 2), mapq=60)
    for k in range(12):             # deletions of two lengths at one position
        a = 14 + k
        add(DEL_POS + 1 - a, "%dM%dD%dM" % (a, 2 if k % 3 else 4, 25), flag=16 * (k % 2), mapq=60)
    for k in range(7):              # every read of the stretch ends at TAIL_POS
        ln = 30 + 4 * k
        add(TAIL_POS + 1 - ln, "%dM" % ln, flag=16 * (k % 2), mapq=60 if k else 1)
    add(TAIL_POS - 20, "40M", flag=1024, mapq=60)       # ... and a duplicate goes on past it only for a caller that forgets the mask
    reads.sort(key=lambda r: r[0])
    return genome, reads


def make_variants(genome, seed=11):
    """[(pos0, ref, alt, af string, has INDEL key, kind)]"""
    rng = np.random.default_rng(seed)
    afs = ["0.000000", "1.000000", "0.001000", "0.010000", "0.050000", "0.200000", "0.500000", "0.950000"]
    g = genome
    var = []
    for p0, (alt, _) in sorted(PLANTED.items()):
        var.append((p0, g[p0], alt, afs[(p0 // 30) % len(afs)], False, "snv_planted"))
    clean = [p for p in range(8, GLEN - 8, 19) if p not in PLANTED and not HOLE[0] - 2 <= p < HOLE[1] + 2]
    for i, p0 in enumerate(clean):
        var.append((p0, g[p0], "ACGT"[("ACGT".index(g[p0]) + 1 + i % 3) % 4], afs[i % len(afs)], False, "snv_clean"))
    b = g[INS_POS]
    var += [(INS_POS, b, b + "AT", "0.300000", False, "ins_match"), (INS_POS, b, b + "AC", "0.300000", False, "ins_match"),
            (INS_POS, b, b + "GG", "0.300000", False, "ins_wrong"), (INS_POS, b, b + "A", "0.300000", False, "ins_wrong"),
            (INS_POS, b, "ACGT"[("ACGT".index(b) + 1) % 4], "0.100000", False, "snv_clean"),
            (INS_POS, b, "ACGT"[("ACGT".index(b) + 2) % 4], "0.300000", True, "indel_key")]
    b = g[INS_N_POS]
    var += [(INS_N_POS, b, b + "AN", "0.050000", False, "ins_match"), (INS_N_POS, b, b + "AA", "0.050000", False, "ins_match"),
            (INS_N_POS, b, b + "AC", "0.050000", False, "ins_wrong")]
    d = DEL_POS
    assert g[d + 1:d + 5] == "NNNN" and g[d] != "N"
    wrong0 = "ACGT"[("ACGT".index(g[d]) + 1) % 4]
    var += [(d, g[d] + "NN", g[d], "0.200000", False, "del_match"), (d, g[d] + "NNNN", g[d], "0.200000", False, "del_match"),
            (d, g[d] + "NNN", g[d], "0.200000", False, "del_wrong"), (d, g[d] + "GA", g[d], "0.200000", False, "del_wrong"),
            (d, g[d] + "nn", g[d], "0.200000", False, "del_wrong"),
            (d, wrong0 + "NN", wrong0, "0.200000", False, "del_ref_disagrees")]     # REF[0] is not part of the key: still a match
    t = TAIL_POS
    var += [(t, g[t], "ACGT"[("ACGT".index(g[t]) + 1) % 4], "0.100000", False, "tails_snv"),
            (t, g[t], "ACGT"[("ACGT".index(g[t]) + 1) % 4], "0.100000", True, "tails_indel_key"),
            (t, g[t:t + 3], g[t], "0.100000", False, "tails_del"),
            (t - 1, g[t - 1], "ACGT"[("ACGT".index(g[t - 1]) + 1) % 4], "0.100000", True, "indel_key"),
            (BARE_POS, g[BARE_POS], "ACGT"[("ACGT".index(g[BARE_POS]) + 1) % 4], "0.100000", False, "uncovered")]
    var.sort(key=lambda v: v[0])
    assert len({(v[0], v[1], v[2], v[4]) for v in var}) == len(var)
    return var


def main():
    genome, reads = make_reads()
    var = make_variants(genome)
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.fa"), "w").write(">chr1\n" + genome + "\n")
        with open(os.path.join(tmp, "t.sam"), "w") as f:
            f.write("@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:chr1\tLN:%d\n" % len(genome))
            for i, (pos0, flag, mapq, cg, seq, q) in enumerate(reads):
                f.write("r%d\t%d\tchr1\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\n" % (i, flag, pos0 + 1, mapq, cg, seq, q))
        subprocess.check_call([mg.LOFREQ, "faidx", "t.fa"], cwd=tmp)
        with open(os.path.join(tmp, "t.bam"), "wb") as f:
            subprocess.check_call([mg.LOFREQ, "alnqual", "-b", "t.sam", "t.fa"], cwd=tmp, stdout=f)
        subprocess.check_call([mg.LOFREQ, "index", "t.bam"], cwd=tmp)
        with open(os.path.join(tmp, "v.vcf"), "w") as f:
            f.write("##fileformat=VCFv4.0\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
            for p0, ref, alt, af, key, _ in var:
                f.write("chr1\t%d\t.\t%s\t%s\t100\tPASS\tDP=100;AF=%s%s\n" % (p0 + 1, ref, alt, af, ";INDEL" if key else ""))
        for name, args in RUNS.items():
            out = subprocess.run([mg.LOFREQ, "uniq"] + args + ["-v", "v.vcf", "-o", "-", "t.bam"], cwd=tmp, check=True,
                                 capture_output=True, text=True).stdout
            got = {}
            for line in out.splitlines():
                if line.startswith("#"):
                    continue
                f = line.split("\t")
                info = f[7].split(";")
                kv = dict(x.split("=") for x in info if "=" in x)
                k = (int(f[1]) - 1, f[3], f[4], "INDEL" in info)
                assert k not in got
                got[k] = {"uq": int(kv["UQ"]) if "UQ" in kv else None, "uniq": "UNIQ" in info, "filter": f[6]}
            assert len(got) == len(var), (name, len(got), len(var))         # --output-all
            res[name] = [got[(v[0], v[1], v[2], v[4])] for v in var]
    variants = [{"pos0": v[0], "ref": v[1], "alt": v[2], "af": v[3], "indel_key": v[4], "kind": v[5],
                 "runs": {name: res[name][i] for name in RUNS}} for i, v in enumerate(var)]
    for x in variants:
        if not x["kind"].startswith("snv"):
            print("  %-18s %4d %-6s %-6s af %s key %d  ->  %s" % (x["kind"], x["pos0"], x["ref"], x["alt"], x["af"], x["indel_key"],
                  "  ".join("%s: uq %s uniq %d %s" % (k, r["uq"], r["uniq"], r["filter"]) for k, r in x["runs"].items())))
    # every kind is there, with the kind of result it was put there for
    by = lambda kind: [x for x in variants if x["kind"] == kind]
    D = lambda x: x["runs"]["default"]
    assert len(by("snv_planted")) >= 5 and len(by("snv_clean")) >= 20
    assert all(D(x)["uq"] is not None for x in by("snv_planted") + by("snv_clean") + by("ins_match") + by("del_match"))
    assert len({D(x)["uq"] for x in by("ins_match") if x["pos0"] == INS_POS}) == 2, "the binary tells the two insertions apart"
    assert all(D(x)["uq"] is not None for x in by("ins_wrong") + by("del_wrong") + by("del_ref_disagrees") + by("indel_key"))
    assert min(D(x)["uq"] for x in by("ins_match")) < min(D(x)["uq"] for x in by("ins_wrong") if x["pos0"] == INS_POS)
    assert len({D(x)["uq"] for x in by("del_match")}) == 2
    assert {D(x)["uq"] for x in by("del_ref_disagrees")} == {D(by("del_match")[0])["uq"]}
    assert len({D(x)["uq"] for x in by("del_wrong")}) == 1 and D(by("del_wrong")[0])["uq"] > max(D(x)["uq"] for x in by("del_match"))
    assert all(r["uq"] is None and not r["uniq"] for x in by("uncovered") for r in x["runs"].values())
    assert all(D(x)["uq"] is not None for x in by("tails_snv"))
    assert all(r["uq"] is None and not r["uniq"] for x in by("tails_indel_key") + by("tails_del") for r in x["runs"].values())
    assert any(x["runs"]["detlim"]["uniq"] for x in variants) and not all(x["runs"]["detlim"]["uniq"] for x in variants)
    assert len({D(x)["filter"] for x in variants}) >= 2, "both outcomes of the multiple-testing correction"
    assert {x["af"] for x in variants} >= {"0.000000", "1.000000"}
    kept = [uniq_filter(r[1], r[2]) for r in reads]
    assert 0 < sum(kept) < len(reads) and {r[2] for r in reads} >= {0, 1, 60, 255}
    assert any("H" in r[3] for r in reads) and any("N" in r[3] for r in reads) and any("S" in r[3] for r in reads)
    fix = {"name": "uniq_reads", "generator": "tests/make_uniq_reads_golden.py", "reference_binary": "lofreq 2.1.4 (dist tgz)",
           "encoding": "reads: [pos0, flag, mapq, cigar, seq, qual (chr(33 + value))]; af: the string written to the VCF (strtof); "
                       "uq: the UQ= value or null; uniq: the UNIQ flag; filter: the FILTER column",
           "runs": RUNS, "mtc": "fdr", "alpha": 0.001, "genome": genome, "reads": [list(r) for r in reads], "variants": variants}
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "uniq_reads.json")
    json.dump(fix, open(path, "w"), separators=(",", ":"))
    size = os.path.getsize(path)
    assert size < 150 * 1024, size
    print("uniq_reads: %d reads (%d after uniq's filter), %d variants, %d bytes" % (len(reads), sum(kept), len(variants), size))


if __name__ == "__main__":
    main()
