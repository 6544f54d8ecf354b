"""Fixture for lfq_readset_encode_bam (tests/golden/bam_write.json) from the reference's own 2.1.4 binary, which `make -C oracle
ref` unpacks to oracle/_ref/bin/lofreq: what `lofreq viterbi`, `lofreq alnqual` and `lofreq indelqual` do to the BYTES of BAM records
whose aux blocks are hand-made -- duplicate tags, tags of the wrong type, B arrays and every other type between them, flags 4 / 256 /
512 / 1024, reads with an insertion, a deletion, both, neither, and indels `lofreq viterbi` moves.  Data only: the contig, the input
records and the records every command wrote, as hex from read_name on, with their core fields.

The input BAM is written here with the standard library (one raw-deflate stream per BGZF block with the BC extra field, and the
empty EOF block), so that the aux bytes reach the binary exactly as they are made; the output is read back the same way.

    python tests/make_bamwrite_golden.py          (LFQ_GOLDEN_OUT: another output directory)
"""
import gzip
import json
import os
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import bam_records as br  # noqa: E402

LOFREQ = os.path.join(ROOT, "oracle", "_ref", "bin", "lofreq")
OUT = os.environ.get("LFQ_GOLDEN_OUT") or os.path.join(HERE, "golden")
SEED = 20261
UNIFORM = (40, 30)                                          # -u 40,30
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

COMMANDS = {            # name -> [(sub-command and its options)], run one after the other
    "viterbi": [("viterbi", [])], "viterbi_k": [("viterbi", ["-k"])],
    "alnqual_r": [("alnqual", ["-r"])], "alnqual": [("alnqual", [])], "alnqual_r_B": [("alnqual", ["-r", "-B"])],
    "alnqual_r_A": [("alnqual", ["-r", "-A"])], "alnqual_e": [("alnqual", ["-e"])],
    "indelqual_uniform": [("indelqual", ["--uniform", "%d,%d" % UNIFORM])], "indelqual_dindel": [("indelqual", ["--dindel"])],
    "chain": [("viterbi", []), ("alnqual", ["-r"]), ("indelqual", ["--dindel"])],
}


def make_genome(rng):
    g = list(rng.choice(list("ACGT"), 700))
    for at, rep in ((60, "AT" * 9), (150, "A" * 11), (240, "CAG" * 7), (330, "T" * 10), (420, "TA" * 8), (510, "G" * 9), (600, "AC" * 8)):
        g[at:at + len(rep)] = rep
    return "".join(g)


REPEATS = ((60, 18, 2), (150, 11, 1), (240, 21, 3), (330, 10, 1), (420, 16, 2), (510, 9, 1), (600, 16, 2))


def make_read(rng, genome, i, shape):
    """a read of 40 .. 70 bases over repeat i: its indels are written at the RIGHT end of the repeat, where `lofreq viterbi` does
    not leave them (shape "x": the whole read is reported off its place)"""
    at, rl, unit = REPEATS[i % len(REPEATS)]
    L = int(rng.integers(40, 53))
    before = int(rng.integers(8, 16))
    p = at - before
    end = before + rl                                       # read offset of the first base behind the repeat
    L = max(L, end + unit + 16)
    if shape == "m":
        ops = [("M", L)]
    elif shape == "i":
        ops = [("M", end), ("I", unit), ("M", L - end - unit)]
    elif shape == "d":
        ops = [("M", end - unit), ("D", unit), ("M", L - end + unit)]
    elif shape == "b":                                      # an insertion in front of the repeat's end, a deletion further on
        ops = [("M", end), ("I", unit), ("M", 6), ("D", 2), ("M", L - end - unit - 6)]
    elif shape == "x":                                      # reported 2 bases to the right of where it lies, its first 2 inserted
        ops = [("I", 2), ("M", L - 2)]
    else:                                                   # "s": soft clips around an insertion
        ops = [("S", 3), ("M", end - 3), ("I", unit), ("M", L - end - unit - 2), ("S", 2)]
    if shape == "s":
        p += 3                                              # (the clipped bases are not aligned)
    seq, x = [], p
    for op, ln in ops:
        if op == "M":
            seq.extend(genome[x:x + ln])
            x += ln
        elif op == "I":
            seq.extend(genome[at:at + ln] if shape != "x" else genome[p:p + ln])        # one more repeat unit
            p += ln if shape == "x" else 0
            x = p
        elif op == "S":
            seq.extend(rng.choice(list("ACGT"), ln))
        else:
            x += ln
    seq = list(seq)
    for j in range(len(seq)):
        if rng.random() < 0.01:
            seq[j] = "ACGT"[int(rng.integers(4))]
    assert len(seq) == L, (shape, len(seq), L)
    return {"pos0": p, "cigar": ops, "letters": "".join(seq), "qual": rng.integers(10, 41, L).astype(np.uint8)}


def aux_variants(l, rng):
    z = lambda tag, byte: br.aux_field(tag, "Z", bytes([byte]) * l)
    i4 = lambda tag, v: br.aux_field(tag, "i", struct.pack("<i", v))
    every = br.one_of_every_type()
    return [
        b"",
        i4("NM", 3) + br.aux_field("MD", "Z", b"10A5") + br.aux_field("AS", "C", b"\x30") + br.aux_field("MC", "Z", b"50M") + i4("XS", 7),
        i4("NM", 1) + br.aux_field("NM", "C", b"\2") + z("lb", 70) + br.aux_field("XX", "A", b"q") + z("lb", 71),     # duplicates
        br.aux_field("lb", "A", b"L") + z("ai", 72) + br.aux_field("ad", "A", b"D"),                                     # wrong types
        i4("BI", 5) + z("BI", 73) + z("BD", 74) + br.aux_field("BD", "c", b"\1"),
        i4("NM", 0) + b"".join(every[:9]) + br.aux_field("MD", "Z", b"60") + z("lb", 75) + b"".join(every[9:]) + z("BI", 76)
        + br.aux_field("AS", "s", b"\1\2"),
        z("lb", 77) + z("ai", 78) + z("ad", 79),                                                                         # all there
        z("ai", 80) + br.aux_field("MC", "H", b"1F") + br.aux_field("AS", "B", ("s", 2, b"\1\0\2\0")),
        z("ad", 81) + i4("ai", 9) + z("ai", 82),
    ]


def make_records(rng, genome):
    reads = []
    shapes = "midbsx"
    flags = {5: 4, 9: 256, 13: 512, 17: 1024, 21: 4 | 1024}
    for i in range(24):
        shape = shapes[i % 6]
        flag = flags.get(i, 0)
        if flag & 4:
            shape = "m"
        r = make_read(rng, genome, i // 5 + i, shape)
        aux = aux_variants(len(r["letters"]), rng)
        r.update(name="q%d" % i, mapq=int(20 + i), reverse=bool(i % 3 == 0), flag_other=flag,
                 aux_raw=aux[(i + i // 18) % len(aux)], seq=[br_code(c) for c in r["letters"]])
        reads.append(r)
    return reads


def br_code(c):
    return "ACGTN".index(c)


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def bgzf(payload):
    out = []
    for a in range(0, len(payload), 0xff00):
        chunk = payload[a:a + 0xff00]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = co.compress(chunk) + co.flush()
        size = 12 + 6 + len(body) + 8
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", size - 1) + body
                   + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    return b"".join(out) + EOF_BLOCK


def write_bam(path, genome, recs):
    text = ("@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:chr1\tLN:%d\n" % len(genome)).encode()
    body = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", 1), struct.pack("<i", 5), b"chr1\0",
            struct.pack("<i", len(genome))]
    data = bytes(recs["data"])
    for r in range(len(recs["pos"])):
        d = data[int(recs["data_off"][r]):int(recs["data_off"][r + 1])]
        p = int(recs["data_off"][r]) + int(recs["l_qname"][r])
        words = struct.unpack_from("<%dI" % int(recs["n_cigar"][r]), data, p)
        rlen = sum(w >> 4 for w in words if (w & 15) in (0, 2, 3, 7, 8))
        pos = int(recs["pos"][r])
        core = struct.pack("<iiBBHHHiiii", 0, pos, int(recs["l_qname"][r]), int(recs["mapq"][r]), reg2bin(pos, pos + max(rlen, 1)),
                           int(recs["n_cigar"][r]), int(recs["flag"][r]), int(recs["l_qseq"][r]), -1, -1, 0)
        body.append(struct.pack("<i", len(core) + len(d)) + core + d)
    open(path, "wb").write(bgzf(b"".join(body)))


def parse_bam(path):
    """-> [dict(name, pos, mapq, n_cigar, flag, l_qname, l_qseq, data)] of the records of a BAM, data = the bytes from read_name on"""
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
        block_size, _ref_id, pos, l_name, mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiiBBHHHi", data, o)
        recs.append({"name": data[o + 36:o + 36 + l_name - 1].decode(), "pos": pos, "mapq": mapq, "n_cigar": n_cigar, "flag": flag,
                     "l_qname": l_name, "l_qseq": l_seq, "data": data[o + 36:o + 4 + block_size]})
        o += 4 + block_size
    return recs


def run(tmp, steps, bam_in, tag):
    cur = bam_in
    for k, (cmd, opts) in enumerate(steps):
        out = os.path.join(tmp, "%s_%d.bam" % (tag, k))
        if cmd == "viterbi":
            subprocess.run([LOFREQ, "viterbi", "-f", "t.fa", "-o", out] + opts + [cur], cwd=tmp, check=True, capture_output=True)
        elif cmd == "alnqual":
            res = subprocess.run([LOFREQ, "alnqual", "-b"] + opts + [cur, "t.fa"], cwd=tmp, check=True, capture_output=True)
            open(out, "wb").write(res.stdout)
        else:
            ref = ["-f", "t.fa"] if "--dindel" in opts else []
            subprocess.run([LOFREQ, "indelqual"] + opts + ref + ["-o", out, cur], cwd=tmp, check=True, capture_output=True)
        cur = out
    return parse_bam(cur)


def main():
    rng = np.random.default_rng(SEED)
    genome = make_genome(rng)
    reads = make_records(rng, genome)
    recs = br.encode(reads, ref=genome.encode(), qname_len=[len(r["name"]) + 1 for r in reads])
    core = lambda rs: [[r["pos"], r["flag"], r["mapq"], r["l_qname"], r["n_cigar"], r["l_qseq"], r["data"].hex()] for r in rs]
    fix = {"name": "bam_write", "reference_binary": "lofreq 2.1.4 (dist tgz)", "genome": genome, "seed": SEED, "uniform": list(UNIFORM),
           "record_fields": ["pos", "flag", "mapq", "l_qname", "n_cigar", "l_qseq", "data (hex, from read_name on)"],
           "commands": {k: ["lofreq %s %s" % (c, " ".join(o)) for c, o in v] for k, v in COMMANDS.items()}, "outputs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "t.fa"), "w").write(">chr1\n" + genome + "\n")
        subprocess.check_call([LOFREQ, "faidx", "t.fa"], cwd=tmp)
        write_bam(os.path.join(tmp, "in.bam"), genome, recs)
        back = parse_bam(os.path.join(tmp, "in.bam"))
        assert [r["name"] for r in back] == [r["name"] for r in reads]
        fix["input"] = core(back)
        for name, steps in COMMANDS.items():
            out = run(tmp, steps, "in.bam", name)
            assert [r["name"] for r in out] == [r["name"] for r in reads], "records out of order or missing"
            fix["outputs"][name] = core(out)
    moved = sum(1 for a, b in zip(fix["input"], fix["outputs"]["viterbi"]) if (a[0], a[4]) != (b[0], b[4]) or a[6][:2 * (a[3] + 4 * a[4])] != b[6][:2 * (b[3] + 4 * b[4])])
    assert moved >= 3, "no read viterbi shifts"
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "bam_write.json")
    json.dump(fix, open(path, "w"), separators=(",", ":"))
    print("bam_write: %d bytes, %d reads, %d moved by viterbi" % (os.path.getsize(path), len(reads), moved))


if __name__ == "__main__":
    main()
