"""Fixture for lfq_bam_index_build (tests/golden/bai_binary.json): the .bai that the reference's own 2.1.4 binary (`make -C oracle
ref` unpacks it to oracle/_ref/bin/lofreq) writes with `lofreq index` -- its bytes, base64; tests/bai_model.py parses them -- for two sorted BAMs of the same reads:

  "python"   the BAM written here (tests/bai_model.py's bgzf_file: stored blocks of mixed sizes that records straddle), kept as its
             gzip-compressed payload and the block cuts, from which bgzf_file makes the same bytes again
  "htslib"   the binary's own output for it, `lofreq indelqual -u 40`: htslib's blocks and streams, records grown by BI / BD
The .bai files are kept gzip-compressed (their linear indices repeat one offset thousands of times).

Five references: chrA beyond 64 Mb with a dense 16 kb window, reads with N skips of 20 kb, 200 kb and 2 Mb and one across an 8 Mb
boundary above 64 Mb; chrB without reads; chrC sparse; chrD dense; chrE with placed unmapped reads only; reads without coordinates
at the end; `lofreq idxstats` of the first.  The generator asserts through the model that the fixture holds every case of rules 4 and 6 it is there for.  Data only.

    python tests/make_bai_golden.py          (LFQ_GOLDEN_OUT: another output directory)
"""
import base64
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import bai_model as bm  # noqa: E402

LOFREQ = os.path.join(ROOT, "oracle", "_ref", "bin", "lofreq")
OUT = os.environ.get("LFQ_GOLDEN_OUT") or os.path.join(HERE, "golden")
SEED = 20262
REFS = [("chrA", 100000000), ("chrB", 50000), ("chrC", 1000000), ("chrD", 300000), ("chrE", 200000)]
L = 50
DENSE_WINDOW = 62                                           # of chrA: 1 015 808 .. 1 032 192, in the 128 kb bin of windows 56 .. 63
PIECES = (700, 65280, 3001, 30000, 1, 12345, 20000, 257, 9000)


def make_records(rng):
    """[(refID, pos, record bytes)] in file order"""
    out = []

    def add(ref_id, pos, cigar, flag=0):
        out.append((ref_id, pos, bm.record(ref_id, pos, cigar, flag, b"q%d" % len(out), len(out))))

    m = [("M", L)]
    w = DENSE_WINDOW << 14
    for pos in (100, 5000, 16000):
        add(0, pos, m)
    add(0, 2 * 131072 + 1000, [("M", 20), ("N", 20000), ("M", 30)])                 # level 4
    add(0, w - 16384 + 100, m)                              # window 61: a 16 kb bin that merges into the 128 kb bin ...
    add(0, w - 16384 + 300, [("S", L)])                     # (all soft clip: one reference base)
    add(0, w - 10, m)                                       # ... which this read, across the windows' edge, makes exist
    dense = np.sort(rng.integers(w, w + 16384 - L, 800))
    for k, pos in enumerate(dense.tolist()):
        if k == 600:
            add(0, pos, [("M", 25), ("N", w + 16384 - pos), ("M", 25)])             # into window 63: the 128 kb bin again, far on
        if k in (100, 700):
            add(0, pos, m, flag=4)                          # placed unmapped: in its bin, not in the linear index
        add(0, pos, m)
    add(0, 3 * 1048576 + 1000, [("M", 25), ("N", 200000), ("M", 25)])               # level 3
    add(0, 2 * 8388608 + 1000, [("M", 25), ("N", 2000000), ("M", 25)])              # level 2
    for pos in (70000000, 70000040, 70020000):
        add(0, pos, m)
    add(0, 9 * 8388608 - 1000, [("M", 25), ("N", 2000), ("M", 25)])                 # across an 8 Mb edge above 64 Mb: bin 2
    for pos in (50000, 200000, 200100):                                             # chrC: windows 3 and 12 alone
        add(2, pos, m)
    for pos in np.sort(rng.integers(0, 290000, 150)).tolist():
        add(3, pos, [("M", 30), ("D", 3), ("M", 20)] if pos % 3 == 0 else m)
    for pos in (1000, 1000, 40000):
        add(4, pos, m, flag=4)
    for _ in range(7):
        add(-1, -1, m, flag=4)
    return out


def index_of(tmp, bam_path):
    """-> the bytes of the .bai the binary writes for the BAM"""
    subprocess.run([LOFREQ, "index", bam_path], cwd=tmp, check=True, capture_output=True)
    return open(bam_path + ".bai", "rb").read()


def check_contents(bam, want):
    """the model gives the binary's index, and the fixture holds the cases it is there for"""
    log = []
    got = bm.build_from_file(bam, log)[0]
    assert got == want, "the model and the binary disagree"
    what = {(e[2], bm.bin_level(e[1])) for e in log if e[2] in ("merged", "no_parent", "wide")}
    assert {("merged", 5), ("no_parent", 5), ("wide", 5)} <= what, sorted(what)
    assert {"join", "apart"} <= {e[2] for e in log}
    windows = [e for e in log if e[1] == "window"]
    assert any(not t and lead for _, _, t, lead in windows) and any(not t and not lead for _, _, t, lead in windows)
    levels = {bm.bin_level(b) for r in want["refs"] for b in r["bins"]}
    assert levels >= {1, 2, 3, 4, 5} and 2 in want["refs"][0]["bins"], sorted(levels)
    assert want["refs"][1] == {"bins": {}, "linear": [], "meta": None} and want["n_no_coor"] == 7
    assert want["refs"][4]["linear"] == [] and want["refs"][4]["meta"][1] == [0, 3]
    return got


def main():
    rng = np.random.default_rng(SEED)
    recs = make_records(rng)
    keys = [(r[0] if r[0] >= 0 else 1 << 30, r[1]) for r in recs]
    assert keys == sorted(keys), "not sorted"
    payload = bm.header(REFS) + b"".join(r[2] for r in recs)
    cuts, at, k = [], 0, 0
    while at + PIECES[k % len(PIECES)] < len(payload):
        at += PIECES[k % len(PIECES)]
        cuts.append(at)
        k += 1
    bam = bm.bgzf_file(payload, cuts)
    fix = {"name": "bai_binary", "reference_binary": "lofreq 2.1.4 (dist tgz)", "seed": SEED, "n_reads": len(recs),
           "refs": [list(r) for r in REFS], "commands": {"python": ["lofreq index in.bam"],
                                                         "htslib": ["lofreq indelqual -u 40 -o out.bam in.bam", "lofreq index out.bam"]}}
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "in.bam"), "wb").write(bam)
        bai = index_of(tmp, os.path.join(tmp, "in.bam"))
        stats = subprocess.run([LOFREQ, "idxstats", "in.bam"], cwd=tmp, check=True, capture_output=True, text=True).stdout
        subprocess.run([LOFREQ, "indelqual", "-u", "40", "-o", "out.bam", "in.bam"], cwd=tmp, check=True, capture_output=True)
        bam2 = open(os.path.join(tmp, "out.bam"), "rb").read()
        bai2 = index_of(tmp, os.path.join(tmp, "out.bam"))
    check_contents(bam, bm.parse_bai(bai))
    got2, data2 = bm.build_from_file(bam2)[:2]
    assert got2 == bm.parse_bai(bai2), "the model and the binary disagree on htslib's blocks"
    assert len(bm.record_chain(data2, bm.parse_header(data2)[0])) - 1 == len(recs)
    fix["idxstats"] = stats
    z = lambda raw: base64.b64encode(gzip.compress(raw, 9, mtime=0)).decode()
    fix["python"] = {"payload_gz_base64": z(payload), "cuts": cuts, "bai_gz_base64": z(bai)}
    fix["htslib"] = {"bam_base64": base64.b64encode(bam2).decode(), "bai_gz_base64": z(bai2)}
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "bai_binary.json")
    json.dump(fix, open(path, "w"), separators=(",", ":"))
    print("bai_binary: %d bytes; %d reads, BAMs of %d and %d bytes" % (os.path.getsize(path), len(recs), len(bam), len(bam2)))


if __name__ == "__main__":
    main()
