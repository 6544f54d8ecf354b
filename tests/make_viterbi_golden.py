"""Fixtures for the viterbi realigner (tests/golden/viterbi_*.json) from the reference's own 2.1.4 binary, which
`make -C oracle ref` unpacks to oracle/_ref/bin/lofreq: seeded reads (tests/viterbi_reads.py) as SAM + FASTA ->
`lofreq viterbi -f t.fa -o out.bam t.sam`, with the default -q (median quality in place of a quality of 2) and with -q 20 ->
position and CIGAR of every record of the BAM it writes.  Data only.

  viterbi_small   a few hundred reads, held inline (contig, reads, results)
  viterbi_shapes  a few thousand, regenerated from the seed: generator parameters and version, SHA-256 of the SAM text, results

The BAM is read with the standard library: BGZF is a series of gzip members, a record's pos, n_cigar_op and CIGAR words are
at fixed offsets.  Records come back in input order (the command writes each read as it has dealt with it).

    python tests/make_viterbi_golden.py          (LFQ_GOLDEN_OUT: another output directory)
"""
import gzip
import json
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import viterbi_reads as vr  # noqa: E402

LOFREQ = os.path.join(ROOT, "oracle", "_ref", "bin", "lofreq")
OUT = os.environ.get("LFQ_GOLDEN_OUT") or os.path.join(HERE, "golden")
DEF_QUALS = [-1, 20]
SMALL = dict(seed=8101, n=320, glen=1500)
SHAPES = dict(seed=8102, n=2400, glen=3000)


def parse_bam(path):
    """[(name, pos0, cigar string)]"""
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
        block_size, _ref_id, pos, l_name, _mapq, _bin, n_cigar = struct.unpack_from("<iiiBBHH", data, o)
        name = data[o + 36:o + 36 + l_name - 1].decode()
        words = struct.unpack_from("<%dI" % n_cigar, data, o + 36 + l_name)
        recs.append((name, pos, "".join("%d%s" % (w >> 4, "MIDNSHP=X"[w & 15]) for w in words) or "*"))
        o += 4 + block_size
    return recs


def run_binary(genome, reads):
    """-> (sha256 of the SAM text, {def_qual: [[pos0, cigar string]]})"""
    text = vr.sam_text(genome, reads)
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.fa"), "w").write(">chr1\n" + genome + "\n")
        open(os.path.join(tmp, "t.sam"), "w").write(text)
        subprocess.check_call([LOFREQ, "faidx", "t.fa"], cwd=tmp)
        for dq in DEF_QUALS:
            out = os.path.join(tmp, "out%d.bam" % dq)
            args = [LOFREQ, "viterbi", "-f", "t.fa", "-o", out] + (["-q", str(dq)] if dq >= 0 else []) + ["t.sam"]
            subprocess.run(args, cwd=tmp, check=True, capture_output=True)
            recs = parse_bam(out)
            assert [n for n, _, _ in recs] == [r["name"] for r in reads], "records out of order or missing"
            res[str(dq)] = [[p, c] for _, p, c in recs]
    return vr.sha256(text), res


def dump(name, fix):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".json")
    json.dump(fix, open(path, "w"), separators=(",", ":"))
    print("%s: %d bytes" % (name, os.path.getsize(path)))


def main():
    for name, params, inline in (("viterbi_small", SMALL, True), ("viterbi_shapes", SHAPES, False)):
        R = vr.make(**params)
        sha, res = run_binary(R["genome"], R["reads"])
        fix = {"name": name, "generator": {"module": "tests/viterbi_reads.py", "version": vr.GENERATOR_VERSION, "params": params},
               "reference_binary": "lofreq 2.1.4 (dist tgz)", "command": "lofreq viterbi -f t.fa [-q Q] -o out.bam t.sam",
               "n_reads": len(R["reads"]), "sam_sha256": sha, "results": res}
        if inline:
            fix["genome"] = R["genome"]
            fix["reads"] = [[r["name"], r["pos0"], "".join("%d%s" % (l, o) for o, l in r["cigar"]), r["seq"],
                             "".join(chr(33 + q) for q in r["qual"]), r["shape"]] for r in R["reads"]]
        dump(name, fix)


if __name__ == "__main__":
    main()
