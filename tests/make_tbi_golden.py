"""Fixture for the .tbi rules (tests/golden/tbi_binary.json) from the reference's own 2.1.4 binary, which `make -C oracle ref` unpacks to
oracle/_ref/bin/lofreq.  Data only.  Per row of tests/tbi_edges.py's BINARY, `lofreq filter --no-defaults -i x.vcf -o o.vcf.gz` is run:

  gz        the binary's own o.vcf.gz, base64 (its block boundaries and compressed sizes are the binary's: they cannot be regenerated)
  tbi       its o.vcf.gz.tbi, inflated and parsed (tbi_model.pack's form: as_json's with the linear indexes run-length coded), or null
            where it wrote none
  status    the exit status; messages: its hts_idx / tbx / vcf_file_close lines on standard error

"note" counts the rows the binary indexed and tbi_model reproduces, and those it wrote no index for and the model refuses.

    python tests/make_tbi_golden.py          (LFQ_GOLDEN_OUT: another output directory)
"""
import base64
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import bai_model as bm  # noqa: E402
import tbi_edges as te  # noqa: E402
import tbi_model as tm  # noqa: E402
import vcf_model as vm  # noqa: E402

LOFREQ = os.path.join(ROOT, "oracle", "_ref", "bin", "lofreq")
OUT = os.environ.get("LFQ_GOLDEN_OUT") or os.path.join(HERE, "golden")


def model_of(gz):
    """tbi_model over the binary's own file -> the parsed index, or (why, line)"""
    text, data_off, comp_off = bm.file_tables(gz)
    try:
        return tm.build(text, data_off, comp_off, 0)
    except vm.Refused as e:
        return (e.why, e.line)


def main():
    assert os.path.exists(LOFREQ), "run `make -C oracle ref` first"
    gold = {"rows": [], "note": ""}
    same = refused = differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name, text in te.BINARY:
            assert max([len(ln) for _, ln in vm.split_lines(text)] or [0]) < 4095, name
            src, dst = os.path.join(tmp, "x.vcf"), os.path.join(tmp, "o.vcf.gz")
            for path in (dst, dst + ".tbi"):
                if os.path.exists(path):
                    os.remove(path)
            open(src, "wb").write(text)
            p = subprocess.run([LOFREQ, "filter", "--no-defaults", "-i", src, "-o", dst], capture_output=True, timeout=120)
            keep = ("hts_idx", "tbx", "vcf_file_close", "[E::", "[W::", "WARNING", "ERROR", "FATAL")
            msgs = [ln.replace(tmp + os.sep, "")[:160] for ln in p.stderr.decode("latin-1").split("\n") if any(k in ln for k in keep)][:6]
            gz = open(dst, "rb").read()
            tbi = None
            if os.path.exists(dst + ".tbi"):
                tbi = tm.as_json(tm.parse_tbi(bm.file_tables(open(dst + ".tbi", "rb").read())[0]))
            got = model_of(gz)
            if tbi is None:
                refused += isinstance(got, tuple)
                differ += not isinstance(got, tuple)
            else:
                same += isinstance(got, dict) and tm.as_json(got) == tbi
                differ += not (isinstance(got, dict) and tm.as_json(got) == tbi)
            gold["rows"].append({"name": name, "gz": base64.b64encode(gz).decode(), "tbi": None if tbi is None else tm.pack(tbi), "status": p.returncode, "messages": msgs})
            print(name, len(gz), "tbi" if tbi else "no tbi", p.returncode, msgs[:2], "model:", got if isinstance(got, tuple) else "index")
    gold["note"] = ("of %d rows the binary indexed %d, all %d reproduced by tests/tbi_model.py; it wrote no index for %d, of which the "
                    "model refuses %d; %d rows differ" % (len(gold["rows"]), sum(r["tbi"] is not None for r in gold["rows"]), same,
                                                         sum(r["tbi"] is None for r in gold["rows"]), refused, differ))
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "tbi_binary.json"), "w") as f:
        json.dump(gold, f, separators=(",", ":"))
    print(gold["note"])


if __name__ == "__main__":
    main()
