"""Fixture for lfq_bgzf_inflate (tests/golden/bgzf_binary.json): a small BAM written by the reference's own 2.1.4 binary (`make -C
oracle ref` unpacks it to oracle/_ref/bin/lofreq) -- `lofreq indelqual --dindel` on the reads of make_bamwrite_golden.py -- stored as
base64 beside the gzip.decompress of it.  These are htslib's own BGZF blocks and deflate streams, not Python's.  Data only.

    python tests/make_bgzf_golden.py          (LFQ_GOLDEN_OUT: another output directory)
"""
import base64
import gzip
import json
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bam_records as br  # noqa: E402
import make_bamwrite_golden as mb  # noqa: E402


def main():
    rng = np.random.default_rng(mb.SEED)
    genome = mb.make_genome(rng)
    reads = mb.make_records(rng, genome)
    recs = br.encode(reads, ref=genome.encode(), qname_len=[len(r["name"]) + 1 for r in reads])
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.fa"), "w").write(">chr1\n" + genome + "\n")
        subprocess.check_call([mb.LOFREQ, "faidx", "t.fa"], cwd=tmp)
        mb.write_bam(os.path.join(tmp, "in.bam"), genome, recs)
        subprocess.run([mb.LOFREQ, "indelqual", "--dindel", "-f", "t.fa", "-o", "out.bam", "in.bam"], cwd=tmp, check=True,
                       capture_output=True)
        bam = open(os.path.join(tmp, "out.bam"), "rb").read()
    data = gzip.decompress(bam)
    assert data[:4] == b"BAM\1" and bam.endswith(mb.EOF_BLOCK)
    fix = {"name": "bgzf_binary", "reference_binary": "lofreq 2.1.4 (dist tgz)", "command": "lofreq indelqual --dindel -f t.fa -o out.bam in.bam",
           "n_reads": len(reads), "bam_base64": base64.b64encode(bam).decode(), "inflated_base64": base64.b64encode(data).decode(),
           "inflated_crc32": zlib.crc32(data)}
    os.makedirs(mb.OUT, exist_ok=True)
    path = os.path.join(mb.OUT, "bgzf_binary.json")
    json.dump(fix, open(path, "w"), separators=(",", ":"))
    print("bgzf_binary: %d bytes; BAM of %d bytes inflates to %d, %d reads" % (os.path.getsize(path), len(bam), len(data), len(reads)))


if __name__ == "__main__":
    main()
