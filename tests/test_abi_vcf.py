"""CPU tests: the host ABI of the VCF entries -- every symbol resolves and is declared in include/lofreq_amd.h with the signature the
ctypes layer uses, the ABI version is still 10, the constants equal tests/vcf_model.py's, and every LFQ_ERR_INVALID case that needs no
device is refused before one is touched."""
import ctypes as C
import os
import re

import vcf_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFQ_ERR_INVALID = -1
SYMBOLS = {
    "lfq_vcf_open": 7, "lfq_vcf_close": 1, "lfq_vcf_n_records": 1, "lfq_vcf_n_lines_behind": 1, "lfq_vcf_header": 4, "lfq_vcf_records": 2,
    "lfq_vcf_filter_vars": 2, "lfq_vcf_uniq_variants": 7, "lfq_vcf_ign_mask": 5, "lfq_vcfset": 6, "lfq_last_vcf_times": 2,
}


def _lib():
    from lofreq_amd import _lib as m
    return m, m.load()


def test_symbols_version_and_declarations():
    m, L = _lib()
    header = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    for s, n_args in SYMBOLS.items():
        assert hasattr(L, s), s
        decl = re.search(r"\b%s\(([^;]*)\);" % s, header)
        assert decl, s
        assert decl.group(1).count(",") + 1 == n_args, s
        assert len(getattr(L, s).argtypes) == n_args, s
    assert L.lfq_abi_version() == 10 and "#define LFQ_ABI_VERSION 10" in header
    for name, v in (("LFQ_VCF_LINE_TOO_LONG", vm.LINE_TOO_LONG), ("LFQ_VCF_NUL", vm.NUL), ("LFQ_VCF_NUMBER", vm.NUMBER),
                    ("LFQ_VCF_FIELDS", vm.FIELDS), ("LFQ_VCF_UNSORTED", vm.UNSORTED), ("LFQ_VCF_INTERVAL", vm.INTERVAL),
                    ("LFQ_VCF_MULTIALLELIC", vm.MULTIALLELIC), ("LFQ_VCF_STREAM", vm.STREAM), ("LFQ_VCF_TABIX", vm.TABIX),
                    ("LFQ_VCFSET_INTERSECT", vm.INTERSECT), ("LFQ_VCFSET_COMPLEMENT", vm.COMPLEMENT), ("LFQ_VCFSET_CONCAT", vm.CONCAT),
                    ("LFQ_VCFSET_DROPPED", vm.DROPPED), ("LFQ_VCFSET_IGNORED", vm.IGNORED), ("LFQ_VCFSET_TAKEN", vm.TAKEN),
                    ("LFQ_VCFSET_WRITTEN", vm.WRITTEN)):
        assert re.search(r"#define %s %d\b" % (name, v), header), name
    for name, v in (("PASSES", vm.F_PASSES), ("FILTERED", vm.F_FILTERED), ("INDEL_LEN", vm.F_INDEL_LEN), ("INDEL_KEY", vm.F_INDEL_KEY),
                    ("ALT_COMMA", vm.F_ALT_COMMA)):
        assert re.search(r"#define LFQ_VCF_F_%s %du\b" % (name, v), header), name
    assert (C.sizeof(m.VcfTable), C.sizeof(m.VcfsetConf), C.sizeof(m.VcfsetResult), C.sizeof(m.VcfTimes)) == (104, 32, 72, 96)
    # the private header states the same values and limits
    priv = open(os.path.join(ROOT, "lofreq_amd", "csrc", "lfq_vcf.h")).read()
    for name, v in (("LFQ_VC_LINE_TOO_LONG", 1), ("LFQ_VC_NUL", 2), ("LFQ_VC_NUMBER", 3), ("LFQ_VC_FIELDS", 4), ("LFQ_VC_UNSORTED", 5),
                    ("LFQ_VC_INTERVAL", 6), ("LFQ_VC_MULTIALLELIC", 7), ("LFQ_VCF_MAX_LINE", vm.MAX_LINE),
                    ("LFQ_VCF_MAX_HEADER_LINES", vm.MAX_HEADER_LINES), ("LFQ_VCF_HEADER_PREFIX_LEN", len(vm.HEADER))):
        assert re.search(r"#define %s %d\b" % (name, v), priv), name


def test_package_exports():
    import lofreq_amd as la
    for name in ("Vcf", "VcfError", "vcfset", "last_vcf_times"):
        assert hasattr(la, name) and name in la.__all__
    e = la.VcfError(vm.MULTIALLELIC, 0, 12)
    assert (e.why, e.file, e.line) == (vm.MULTIALLELIC, 0, 12) and isinstance(e, ValueError)


def test_refusals_without_a_device():
    m, L = _lib()
    h, why, line = C.c_void_p(), C.c_int(-7), C.c_int64(-7)
    data = b"c1\t1\t.\tA\tC\n"
    assert L.lfq_vcf_open(None, data, len(data), 0, C.byref(h), C.byref(why), C.byref(line)) == LFQ_ERR_INVALID
    assert (why.value, line.value) == (0, 0)            # a refused CALL names no line
    assert L.lfq_vcf_open(None, data, len(data), 0, C.byref(h), None, None) == LFQ_ERR_INVALID
    L.lfq_vcf_close(None)
    assert L.lfq_vcf_n_records(None) == 0 and L.lfq_vcf_n_lines_behind(None) == 0
    p, n, found = C.c_void_p(), C.c_int64(0), C.c_int(0)
    assert L.lfq_vcf_header(None, C.byref(p), C.byref(n), C.byref(found)) == LFQ_ERR_INVALID
    t = m.VcfTable()
    assert L.lfq_vcf_records(None, C.byref(t)) == LFQ_ERR_INVALID
    assert L.lfq_vcf_filter_vars(None, None) == LFQ_ERR_INVALID
    v, lines, bad = m.UniqVariants(), C.c_void_p(), C.c_int64(-7)
    assert L.lfq_vcf_uniq_variants(None, b"c1", 1, 0.0, C.byref(v), C.byref(lines), C.byref(bad)) == LFQ_ERR_INVALID and bad.value == 0
    assert L.lfq_vcf_ign_mask(None, b"c1", 10, None, None) == LFQ_ERR_INVALID
    conf = m.VcfsetConf(0, 0, 0, 0, 0, 0, None)
    out = C.POINTER(m.VcfsetResult)()
    assert L.lfq_vcfset(None, None, None, 0, C.byref(conf), C.byref(out)) == LFQ_ERR_INVALID
    assert L.lfq_vcfset(None, None, None, -1, C.byref(conf), C.byref(out)) == LFQ_ERR_INVALID
    assert L.lfq_vcfset(None, None, None, 0, None, None) == LFQ_ERR_INVALID
    assert L.lfq_last_vcf_times(None, None) == LFQ_ERR_INVALID
