"""Fixture for -l / --bed (tests/golden/bed_binary.json) from the reference's own 2.1.4 binary, which `make -C oracle ref` unpacks
to oracle/_ref/bin/lofreq.  Data only.

  reads   two contigs, c1 (600 bp) and c2 (400 bp), a few hundred reads: M, D, N, I, soft clips, one read that is all clip, both
          strands; SNVs planted inside the targets and in their flanks; on c2 a stack of six 10M reads followed by six 50M reads
          at one position (the order of -l and -d: with a target 20 bases in and -d 3, the 10M reads use up none of the cap).
  beds    BED texts: plain, unsorted, overlapping and duplicate lines, both formats mixed, track / browser / # lines, tabs and runs
          of blanks, \\r\\n, the empty-line cut-off, a zero-length line, a name not in the BAM, a contig with no line, and the four
          parse errors.  Per text the columns `plpsummary -l` prints with their base counts (or the binary's exit status), for
          some the VCF lines and the test count of `call -l --no-default-filter` and the columns of `plpsummary -l`, with and
          without -d.
  nobed   the columns of `plpsummary` without -l, and under each -d without -l (what the cap does when the BED does not go first).

    python tests/make_bed_golden.py          (LFQ_GOLDEN_OUT: another output directory)
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
CONTIGS = (("c1", 600), ("c2", 400))
# planted alternatives, in every third read that covers them: inside targets of the plain BED and in their flanks
ALT = {"c1": {120: "T", 150: "G", 205: "C", 260: "A", 330: "T", 470: "G"}, "c2": {60: "A", 140: "C", 325: "G"}}

BEDS = [
    ("plain", "c1\t100\t160\nc1\t250\t300\nc1\t450\t480\nc2\t50\t80\nc2\t320\t330\n", True),
    ("unsorted", "c2\t320\t330\nc1\t450\t480\nc1\t100\t160\nc2\t50\t80\nc1\t250\t300\n", False),
    ("overlapping_and_duplicate", "c1\t100\t160\nc1\t140\t210\nc1\t100\t160\nc1\t100\t120\nc1\t90\t400\nc1\t395\t399\nc2\t50\t80\nc2\t50\t80\n", True),
    ("both_formats", "c1\t100\t160\nc1 206\nc1 261 rs5\nc1 331.5 400\nc2 +61\nc2\t320\t330\n", True),
    ("track_browser_comment", "track name=targets description=\"x\"\nbrowser position c1:1-100\n# a comment\n  # another\nc1\t100\t160\n"
                              "browser 7 3\ntrack 0\nc2\t50\t80\n", False),
    ("tabs_and_blanks", "  c1   100 \t 160  extra fields 7 8\n\tc1\t\t250\t\t300\n   \t \nc2 50    80\n", False),
    ("crlf", "c1\t100\t160\r\nc1\t250\t300\r\n\r\nc2\t50\t80\r\n", False),
    ("empty_line_cut_off", "c1\t100\t160\n\nc1\t250\t300\nc2\t50\t80\n", False),
    ("empty_first_line", "\nc1\t100\t160\n", False),
    ("zero_length", "c1\t130\t130\nc1\t250\t300\nc2\t325\t325\n", True),
    ("name_not_in_bam", "c9\t0\t1000\nc1\t100\t160\n", False),
    ("contig_without_line", "c1\t100\t160\nc1\t250\t300\n", True),
    ("no_final_newline", "c1\t100\t160\nc2\t50\t80", False),
    ("whole_contigs", "c1\t0\t600\nc2\t0\t400\n", True),
    ("error_no_number", "c1\t100\t160\nc1\tabc\t5\n", False),
    ("error_end_below_beg", "c1\t100\t160\nc2\t80\t50\n", False),
    ("error_list_zero", "c1\t100\t160\nc1\t0\n", False),
    ("error_negative", "c1 -5 7\n", False),
]
CALL_CAPS = [None, 3, 10]


def make_reads(seed=29):
    rng = np.random.default_rng(seed)
    genome = {name: "".join(rng.choice(list("ACGT"), n)) for name, n in CONTIGS}
    spec = []                                                   # (contig, pos0, cigar)
    shapes = ["70M", "5S65M", "60M10S", "30M4D36M", "25M40N35M", "33M2I35M", "20M1D20M1I29M", "8S40M3D22M"]
    for name, n in CONTIGS:
        starts = np.sort(rng.integers(0, n - 110, 170 if name == "c1" else 90))
        for k, p in enumerate(starts.tolist()):
            spec.append((name, p, shapes[int(rng.integers(0, len(shapes)))] if k % 4 == 0 else "70M"))
    spec.append(("c1", 128, "30S"))                             # all clip: no reference base, bam_endpos = pos + 1
    spec.append(("c1", 500, "30S"))
    spec += [("c2", 300, "10M")] * 6 + [("c2", 300, "50M")] * 6  # the -l / -d order
    order = {name: i for i, (name, _) in enumerate(CONTIGS)}
    spec = sorted(enumerate(spec), key=lambda t: (order[t[1][0]], t[1][1], t[0]))      # stable: the stack keeps its order
    reads = []
    for k, (_, (name, pos0, cg)) in enumerate(spec):
        seq, x = [], pos0
        for n, op in [(int(a), b) for a, b in re.findall(r"(\d+)([MIDNS])", cg)]:
            if op == "M":
                for j in range(n):
                    b = genome[name][x + j]
                    if x + j in ALT[name] and k % 3 == 0:
                        b = ALT[name][x + j]
                    seq.append(b)
                x += n
            elif op in "IS":
                seq.extend(rng.choice(list("ACGT"), n))
            else:
                x += n
        qual = "".join(chr(33 + int(q)) for q in rng.integers(28, 41, len(seq)))
        reads.append([name, pos0, 16 if k % 3 == 1 else 0, 60, cg, "".join(seq), qual])
    return genome, reads


def write_inputs(tmp, genome, reads):
    with open(os.path.join(tmp, "t.fa"), "w") as f:
        for name, _ in CONTIGS:
            f.write(">%s\n%s\n" % (name, genome[name]))
    with open(os.path.join(tmp, "t.sam"), "w") as f:
        f.write("@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS))
        for i, (name, pos0, flag, mapq, cg, seq, q) in enumerate(reads):
            f.write("r%d\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\n" % (i, flag, name, pos0 + 1, mapq, cg, seq, q))
    subprocess.check_call([mg.LOFREQ, "faidx", "t.fa"], cwd=tmp)


def plp_columns(tmp, extra):
    """-> (exit status, [[contig, pos0, bases in the column], ...])"""
    r = subprocess.run([mg.LOFREQ, "plpsummary", "-f", "t.fa"] + extra + ["t.sam"], cwd=tmp, capture_output=True, text=True)
    cols = []
    for line in r.stdout.splitlines():
        if line.strip() and not line.startswith(" ") and not line.startswith("\t"):
            f = line.split("\t")
            if len(f) > 8 and f[1].isdigit():
                nb = sum(int(x) for tok in f[4:9] for x in tok.split(":")[1].split("/"))
                cols.append([f[0], int(f[1]) - 1, nb])
    return r.returncode, cols


def pack(cols, with_nb):
    """[[contig, pos0, bases]] in the binary's order -> {"ranges": {contig: [[first, behind the last], ...]}, "nb": {contig: [...]}}"""
    out = {"ranges": {}}
    if with_nb:
        out["nb"] = {}
    for name, pos0, nb in cols:
        r = out["ranges"].setdefault(name, [])
        if r and r[-1][1] == pos0:
            r[-1][1] = pos0 + 1
        else:
            assert not r or r[-1][1] < pos0
            r.append([pos0, pos0 + 1])
        if with_nb:
            out["nb"].setdefault(name, []).append(nb)
    return out


def plp_columns_of(genome, reads, extra):
    with tempfile.TemporaryDirectory() as tmp:
        write_inputs(tmp, genome, reads)
        st, cols = plp_columns(tmp, extra)
        assert st == 0
        return cols


def call(tmp, extra):
    env = dict(os.environ)
    env["PATH"] = os.path.dirname(os.path.abspath(mg.LOFREQ)) + ":" + env["PATH"]
    out = os.path.join(tmp, "out.vcf")
    if os.path.exists(out):
        os.remove(out)
    res = subprocess.run([mg.LOFREQ, "call", "-f", "t.fa", "-o", "out.vcf", "--no-default-filter"] + extra + ["t.sam"], cwd=tmp,
                         check=True, capture_output=True, text=True, env=env)
    ntests = None
    for line in res.stderr.splitlines():
        if "tests performed" in line and "indel" not in line:
            ntests = int(line.split(":")[-1])
    return [l for l in open(out).read().splitlines() if not l.startswith("#")], ntests


def main():
    genome, reads = make_reads()
    beds = []
    with tempfile.TemporaryDirectory() as tmp:
        write_inputs(tmp, genome, reads)
        st, nobed = plp_columns(tmp, [])
        assert st == 0 and nobed
        for name, text, with_calls in BEDS:
            with open(os.path.join(tmp, "t.bed"), "wb") as f:
                f.write(text.encode("latin-1"))
            st, cols = plp_columns(tmp, ["-l", "t.bed"])
            row = {"name": name, "text": text, "status": st}
            if st == 0:
                row["columns"] = pack(cols, False)
            if with_calls and st == 0:
                row["calls"] = []
                for d in CALL_CAPS:
                    cap = ["-d", str(d)] if d is not None else []
                    vcf, nt = call(tmp, ["-l", "t.bed"] + cap)
                    st_d, cols_d = plp_columns(tmp, ["-l", "t.bed"] + cap)
                    assert st_d == 0
                    row["calls"].append({"max_depth": d, "vcf": vcf, "num_snv_tests": nt, "columns": pack(cols_d, True)})
            beds.append(row)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "bed_binary.json")
    nocap = [{"max_depth": d, "columns": pack(plp_columns_of(genome, reads, ["-d", str(d)]), True)} for d in CALL_CAPS if d is not None]
    json.dump({"name": "bed_binary", "nobed_capped": nocap, "generator": "tests/make_bed_golden.py", "reference_binary": "lofreq 2.1.4 (dist tgz)",
               "contigs": [list(c) for c in CONTIGS], "genome": genome, "reads": reads, "nobed_columns": pack(nobed, True), "beds": beds},
              open(path, "w"), separators=(",", ":"))
    print("bed_binary: %d bytes, %d reads, %d columns without a BED" % (os.path.getsize(path), len(reads), len(nobed)))
    for b in beds:
        print("  %-28s status %d  columns %s  calls %s" % (b["name"], b["status"],
                                                          sum(e - a for v in b.get("columns", {"ranges": {}})["ranges"].values() for a, e in v),
                                                          [(c["max_depth"], len(c["vcf"]), c["num_snv_tests"]) for c in b.get("calls", [])]))


if __name__ == "__main__":
    main()
