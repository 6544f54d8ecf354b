"""Fixture for the VCF rules and `lofreq vcfset` (tests/golden/vcf_binary.json) from the reference's own 2.1.4 binary, which
`make -C oracle ref` unpacks to oracle/_ref/bin/lofreq.  Data only: inputs, the binary's outputs and exit statuses; a text of more
than 400 bytes is held as its SHA-1, length, newline count and longest line (pack), the rows' inputs being tests/vcf_edges.py's.

  roundtrip  VCF texts (latin-1 strings) read and rewritten record by record with no index: `lofreq vcfset -a concat -1 x.vcf` and
             `lofreq filter --no-defaults -i x.vcf` (which turns a FILTER of at most one byte into PASS, lofreq_filter.c:1308-1315).
  sets       the vcfset rows of tests/vcf_edges.py that fit the size limit: options, both texts, the binary's output, status and
             messages.  The second file is written as BGZF with a .tbi built HERE, in Python (the library neither reads nor writes
             one): magic, n_ref, format 2, columns 1 / 2 / 0, meta '#', skip 0, names, then bins, chunks and the 16 kb linear index per
             name, itself BGZF-compressed.  "note" says whether the binary took that index.

    python tests/make_vcf_golden.py          (LFQ_GOLDEN_OUT: another output directory)
"""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import bai_model as bm  # noqa: E402
import vcf_edges as ve  # noqa: E402
import vcf_model as vm  # noqa: E402
from test_fasta_model import bgzf_tables  # noqa: E402

LOFREQ = os.path.join(ROOT, "oracle", "_ref", "bin", "lofreq")
OUT = os.environ.get("LFQ_GOLDEN_OUT") or os.path.join(HERE, "golden")
MAX_TEXT = 9000                # a row's texts together: the fixture stays far below the size limit for a committed file


def bgzf(payload, block=60000):
    return bm.bgzf_file(payload, list(range(block, len(payload), block))) if payload else bm.EOF_BLOCK


def tbi_of(text, comp):
    """the .tbi of the BGZF file `comp`, whose inflated bytes are `text`"""
    comp_off, data_off, _ = bgzf_tables(comp)
    names, per = [], {}
    at = 0
    for s, ln in vm.split_lines(text):
        end_line = s + len(ln) + 1
        if ln[:1] != b"#" and ln.count(b"\t") >= 4:
            f = ln.split(b"\t")
            beg = vm.c_atol(f[1], 18)[0] - 1
            end = beg + max(len(f[3]), 1)
            if f[0] not in per:
                names.append(f[0])
                per[f[0]] = ({}, {})
            bins, lin = per[f[0]]
            v0, v1 = bm.voffset(s, data_off, comp_off), bm.voffset(min(end_line, len(text)), data_off, comp_off)
            b = bm.reg2bin(max(beg, 0), max(end, 1))
            chunks = bins.setdefault(b, [])
            if chunks and chunks[-1][1] == v0:
                chunks[-1][1] = v1
            else:
                chunks.append([v0, v1])
            for w in range(max(beg, 0) >> 14, (max(end, 1) - 1 >> 14) + 1):
                lin.setdefault(w, v0)
        at = end_line
    nm = b"".join(n + b"\0" for n in names)
    out = b"TBI\1" + struct.pack("<8i", len(names), 2, 1, 2, 0, ord("#"), 0, len(nm)) + nm
    for n in names:
        bins, lin = per[n]
        out += struct.pack("<i", len(bins))
        for b in sorted(bins):
            out += struct.pack("<Ii", b, len(bins[b])) + b"".join(struct.pack("<QQ", *c) for c in bins[b])
        n_intv = max(lin) + 1 if lin else 0
        offs, last = [], 0
        for w in range(n_intv):
            last = lin.get(w, last)
            offs.append(last)
        out += struct.pack("<i", n_intv) + b"".join(struct.pack("<Q", o) for o in offs)
    return bgzf(out)


def pack(text, limit=400):
    """a text as the fixture holds it: itself (latin-1) up to `limit` bytes, else its SHA-1, length, newlines and longest line"""
    if len(text) <= limit:
        return text.decode("latin-1")
    return {"sha1": hashlib.sha1(text).hexdigest(), "len": len(text), "newlines": text.count(b"\n"), "longest": max(map(len, text.split(b"\n")))}


def run(args):
    p = subprocess.run([LOFREQ] + args, capture_output=True, timeout=120)
    keep = ("Parsed ", "Wrote ", "FATAL", "ERROR")
    return p.returncode, p.stdout, [ln[:100] for ln in p.stderr.decode("latin-1").split("\n") if ln.startswith(keep)][:8]


def main():
    assert os.path.exists(LOFREQ), "run `make -C oracle ref` first"
    gold = {"roundtrip": [], "sets": [], "note": ""}
    with tempfile.TemporaryDirectory() as tmp:
        for r in ve.OPEN:
            if r["mode"] != vm.STREAM or len(r["data"]) > MAX_TEXT:
                continue
            one = os.path.join(tmp, "rt.vcf")
            open(one, "wb").write(r["data"])
            empty = os.path.join(tmp, "empty.vcf")         # the binary wants a second file for concat
            open(empty, "wb").close()
            st, out, err = run(["vcfset", "--verbose", "-a", "concat", "-1", one, empty])
            st2, out2, err2 = run(["filter", "--no-defaults", "-i", one])
            gold["roundtrip"].append({"name": r["name"], "text": pack(r["data"], 0), "concat": {"status": st, "out": pack(out, 200), "messages": err},
                                      "filter": {"status": st2, "out": pack(out2, 300), "messages": err2}})
        taken = rejected = 0
        for r in ve.SETS:
            texts = [r["one"], r["two"] or b""] + r["more"]
            if sum(len(t) for t in texts) > MAX_TEXT:
                continue
            c = r["conf"]
            paths = []
            for i, t in enumerate(texts):
                paths.append(os.path.join(tmp, "f%d.vcf" % i))
                open(paths[-1], "wb").write(t)
            args = ["vcfset", "--verbose", "-a", ["intersect", "complement", "concat"][c["op"]], "-1", paths[0]]
            if c["op"] != vm.CONCAT:
                comp = bgzf(r["two"])
                open(paths[1] + ".gz", "wb").write(comp)
                open(paths[1] + ".gz.tbi", "wb").write(tbi_of(r["two"], comp))
                args += ["-2", paths[1] + ".gz"]
            for flag in ("only_passed", "only_pos", "only_snvs", "only_indels", "count_only"):
                args += ["--" + flag.replace("_", "-")] if c[flag] else []
            args += ["-I", c["add"].decode()] if c["add"] else []
            args += (paths[2:] or [paths[1]]) if c["op"] == vm.CONCAT else []      # (concat alone: the empty second file stands in)
            st, out, err = run(args)
            if c["op"] != vm.CONCAT:
                bad = any("index" in m.lower() or "tabix" in m.lower() for m in err) and st != 0 and "why" not in ve.expected_set(r)
                rejected += bad
                taken += not bad
            gold["sets"].append({"name": r["name"], "conf": {k: (v.decode("latin-1") if isinstance(v, bytes) else v) for k, v in c.items()},
                                 "one": pack(r["one"], 0), "two": None if r["two"] is None else pack(r["two"], 0),
                                 "more": [pack(m, 0) for m in r["more"]], "status": st, "out": pack(out, 200), "messages": err})
        gold["note"] = ("the binary took the Python-written .tbi in %d intersect / complement rows and rejected it in %d" % (taken, rejected))
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "vcf_binary.json"), "w") as f:
        json.dump(gold, f, separators=(",", ":"))
    print(gold["note"], len(gold["roundtrip"]), len(gold["sets"]))


if __name__ == "__main__":
    main()
