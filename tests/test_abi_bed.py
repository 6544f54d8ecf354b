"""CPU tests: the host ABI of the targets (lfq_bed_parse, lfq_bed_free, lfq_bed_n_names, lfq_bed_name, lfq_bed_intervals,
lfq_bed_overlap) through ctypes against tests/bed_model.py, every LFQ_ERR_INVALID case, lfq_set_bed without a context, the
declarations, the ABI version and the sizes of the structs the feature must not touch.  No device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bed_edges as be
import bed_model as bm
from test_bed_model import FX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFQ_ERR_INVALID = -1


def _parse(L, text):
    raw = text.encode("latin-1")
    h, bad = C.c_void_p(), C.c_int64(-7)
    rc = L.lfq_bed_parse(raw, len(raw), C.byref(h), C.byref(bad))
    return rc, h, int(bad.value)


def _tables(L, h):
    """-> {name: [(beg, end), ...]} in the library's order of names and intervals"""
    out = {}
    for i in range(L.lfq_bed_n_names(h)):
        name = L.lfq_bed_name(h, i)
        beg, end, n = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.c_int64(-1)
        assert L.lfq_bed_intervals(h, name, C.byref(beg), C.byref(end), C.byref(n)) == 0
        out[name.decode("latin-1")] = [(int(beg[k]), int(end[k])) for k in range(n.value)]
    return out


def _texts():
    t = [(r.name, r.text) for r in be.ROWS] + [(n, x) for n, x, _ in be.ACCEPTED_ODD]
    return t + [(b["name"], b["text"]) for b in FX["beds"] if b["status"] == 0]


def test_parse_and_intervals_equal_the_model():
    from lofreq_amd import _lib
    L = _lib.load()
    for name, text in _texts():
        rc, h, bad = _parse(L, text)
        assert rc == 0 and h.value and bad == 0, name
        want = bm.parse(text)
        got = _tables(L, h)
        assert got == want and list(got) == list(want), name         # names in order of first appearance
        assert L.lfq_bed_name(h, -1) is None and L.lfq_bed_name(h, len(want)) is None
        L.lfq_bed_free(h)


def test_overlap_equals_the_model():
    from lofreq_amd import _lib
    L = _lib.load()
    for row in be.ROWS:
        rc, h, _ = _parse(L, row.text)
        assert rc == 0
        got = [L.lfq_bed_overlap(h, row.contig.encode(), b, e) for b, e in row.queries]
        assert got == be.expected(row), row.name
        assert L.lfq_bed_overlap(h, b"no_such_name", 0, 1 << 40) == 0
        L.lfq_bed_free(h)
    # queries beyond 32 bits are taken as they are
    rc, h, _ = _parse(L, "c1\t0\t%d\n" % bm.INT32_MAX)
    assert L.lfq_bed_overlap(h, b"c1", bm.INT32_MAX, bm.INT32_MAX + 1) == 0
    assert L.lfq_bed_overlap(h, b"c1", bm.INT32_MAX - 1, 1 << 40) == 1
    assert L.lfq_bed_overlap(h, b"c1", -5, 0) == 0 and L.lfq_bed_overlap(h, b"c1", -5, 1) == 1
    L.lfq_bed_free(h)


def test_refused_texts_are_lfq_err_invalid_with_the_line():
    from lofreq_amd import _lib
    L = _lib.load()
    rows = [(n, t, line) for n, t, line in be.REFUSED]
    rows += [(b["name"], b["text"], b["text"].count("\n")) for b in FX["beds"] if b["status"] != 0]
    assert len(rows) >= 14
    for name, text, line in rows:
        rc, h, bad = _parse(L, text)
        assert rc == LFQ_ERR_INVALID and not h.value and bad == line, name
        raw = text.encode("latin-1")
        h2 = C.c_void_p(1)
        assert L.lfq_bed_parse(raw, len(raw), C.byref(h2), None) == LFQ_ERR_INVALID and not h2.value     # bad_line may be NULL


def test_invalid_arguments():
    from lofreq_amd import _lib
    L = _lib.load()
    h, bad = C.c_void_p(), C.c_int64(0)
    assert L.lfq_bed_parse(b"c1\t1\t2\n", 7, None, C.byref(bad)) == LFQ_ERR_INVALID
    assert L.lfq_bed_parse(b"c1\t1\t2\n", -1, C.byref(h), C.byref(bad)) == LFQ_ERR_INVALID
    assert L.lfq_bed_parse(None, 5, C.byref(h), C.byref(bad)) == LFQ_ERR_INVALID and bad.value == 0
    assert L.lfq_bed_parse(None, 0, C.byref(h), None) == 0 and L.lfq_bed_n_names(h) == 0      # no text: no targets
    beg, end, n = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.c_int64(-1)
    assert L.lfq_bed_intervals(h, b"c1", C.byref(beg), C.byref(end), C.byref(n)) == 0 and n.value == 0 and not beg and not end
    for args in ((None, b"c1", C.byref(beg), C.byref(end), C.byref(n)), (h, None, C.byref(beg), C.byref(end), C.byref(n)),
                 (h, b"c1", None, C.byref(end), C.byref(n)), (h, b"c1", C.byref(beg), None, C.byref(n)),
                 (h, b"c1", C.byref(beg), C.byref(end), None)):
        assert L.lfq_bed_intervals(*args) == LFQ_ERR_INVALID
    assert L.lfq_bed_overlap(None, b"c1", 0, 10) == 0 and L.lfq_bed_overlap(h, None, 0, 10) == 0
    assert L.lfq_bed_n_names(None) == 0 and L.lfq_bed_name(None, 0) is None
    L.lfq_bed_free(h)
    L.lfq_bed_free(None)
    # lfq_set_bed needs a context, and a name with a BED
    rc, h, _ = _parse(L, "c1\t1\t2\n")
    assert L.lfq_set_bed(None, h, b"c1") == LFQ_ERR_INVALID
    assert L.lfq_set_bed(None, None, None) == LFQ_ERR_INVALID
    L.lfq_bed_free(h)


def test_python_layer():
    import lofreq_amd as la
    b = la.Bed.parse(FX["beds"][0]["text"])
    want = bm.parse(FX["beds"][0]["text"])
    assert b.names == list(want)
    for name, iv in want.items():
        beg, end = b.intervals(name)
        assert beg.dtype == np.int32 and list(zip(beg.tolist(), end.tolist())) == iv
        assert b.overlap(name, iv[0][0], iv[0][0] + 1) and not b.overlap(name, iv[0][0] - 1, iv[0][0])
    assert b.intervals("nope")[0].size == 0 and not b.overlap("nope", 0, 10 ** 9)
    b.close()
    with pytest.raises(la.BedError) as e:
        la.Bed.parse(b"c1\t1\t2\nc1 0\n")
    assert e.value.line == 2
    assert callable(la.SnvCaller.set_bed)


def test_the_new_symbols_are_declared_bound_and_exported():
    from lofreq_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    for decl in ("int lfq_bed_parse(const char *text, int64_t n_bytes, lfq_bed **bed_out, int64_t *bad_line_or_null);",
                 "void lfq_bed_free(lfq_bed *bed);", "int64_t lfq_bed_n_names(const lfq_bed *bed);",
                 "const char *lfq_bed_name(const lfq_bed *bed, int64_t i);",
                 "int lfq_bed_intervals(const lfq_bed *bed, const char *name, const int32_t **beg_out, const int32_t **end_out, "
                 "int64_t *n_out);", "int lfq_bed_overlap(const lfq_bed *bed, const char *name, int64_t beg, int64_t end);",
                 "int lfq_set_bed(lfq_ctx *ctx, const lfq_bed *bed_or_null, const char *name_or_null);"):
        assert decl in hdr, decl
    for sym in ("lfq_bed_parse", "lfq_bed_free", "lfq_bed_n_names", "lfq_bed_name", "lfq_bed_intervals", "lfq_bed_overlap",
                "lfq_set_bed"):
        assert sym in _lib.EXPORTS and hasattr(L, sym), sym
    region_h = open(os.path.join(ROOT, "integration", "lofreq_amd_region.h")).read()
    region_c = open(os.path.join(ROOT, "integration", "lofreq_amd_region.c")).read()
    assert "int lfq_region_set_bed(lfq_region *r, const lfq_bed *bed_or_null);" in region_h
    assert "int lfq_region_set_bed(lfq_region *r, const lfq_bed *bed_or_null)\n{" in region_c
    assert "bed" not in re.search(r"typedef struct lfq_region_opts \{.*?\} lfq_region_opts;", region_h, re.S).group(0)
    for text in (hdr, region_h, open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        assert "BED overlap stays with the caller" not in text


def test_abi_version_is_10_everywhere():
    from lofreq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    assert int(re.search(r"#define LFQ_ABI_VERSION (\d+)", hdr).group(1)) == 10
    assert _lib.LFQ_ABI_VERSION == 10
    assert _lib.load().lfq_abi_version() == 10


# sizeof on x86-64 of the structs callers were compiled against, before this feature
SIZES = {"lfq_region_opts": 48, "lfq_bam_scan_opts": 40, "lfq_kernel_times": 32, "lfq_baq_times": 24, "lfq_baq_fill_stats": 56,
         "lfq_viterbi_times": 24, "lfq_indelqual_times": 24, "lfq_sites_times": 40, "lfq_summary_times": 32,
         "lfq_plp_quals_times": 32, "lfq_bam_decode_times": 56, "lfq_bam_encode_times": 56, "lfq_bgzf_times": 56,
         "lfq_bgzf_deflate_times": 56, "lfq_bam_index_times": 72, "lfq_conf": 80, "lfq_tracks": 96, "lfq_pileup_reads": 104,
         "lfq_pileup_indel_tags": 48}


def test_struct_sizes_are_unchanged(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lofreq_amd_region.h"\nint main(void)\n{\n'
                   + "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (t, t) for t in SIZES) + "    return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call([cc, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"), str(src), "-o", exe])
    got = dict((a, int(b)) for a, b in (l.split() for l in subprocess.check_output([exe], text=True).splitlines()))
    assert got == SIZES
    from lofreq_amd import _lib
    assert C.sizeof(_lib.BaqTimes) == 24 and C.sizeof(_lib.BamScanOpts) == 40 and C.sizeof(_lib.SummaryTimes) == 32
