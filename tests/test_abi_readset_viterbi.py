"""CPU tests: the ABI of lfq_readset_viterbi -- the symbol is declared, bound and exported, the three ABI numbers agree at 10,
the read-level binding declares its option, and the release library still reads its ten environment variables.  No compute."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_new_symbols_are_declared_bound_and_exported():
    from lofreq_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    m = re.search(r"int lfq_readset_viterbi\(lfq_ctx \*ctx, lfq_readset \*rs, int def_qual, lfq_readset \*\*out,\s*"
                  r"const lfq_viterbi_result \*\*result_or_null, const int64_t \*\*order_or_null\);", hdr)
    assert m, "include/lofreq_amd.h does not declare lfq_readset_viterbi as specified"
    assert "lfq_readset_viterbi" in _lib.EXPORTS and hasattr(L, "lfq_readset_viterbi")
    assert L.lfq_readset_viterbi.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p),
                                              C.POINTER(C.POINTER(_lib.ViterbiResult)), C.POINTER(C.c_void_p)]
    from lofreq_amd import pileup, viterbi
    assert callable(pileup.ReadSet.viterbi) and callable(viterbi.readset_viterbi) and callable(viterbi.result_arrays)
    # NULL arguments are refused before anything touches a device
    assert L.lfq_readset_viterbi(None, None, -1, None, None, None) == -1
    region_h = open(os.path.join(ROOT, "integration", "lofreq_amd_region.h")).read()
    region_c = open(os.path.join(ROOT, "integration", "lofreq_amd_region.c")).read()
    assert "int lfq_region_set_viterbi(lfq_region *r, int on, int def_qual);" in region_h
    assert "int lfq_region_set_viterbi(lfq_region *r, int on, int def_qual)\n{" in region_c
    assert "viterbi" not in re.search(r"typedef struct lfq_region_opts \{.*?\} lfq_region_opts;", region_h, re.S).group(0)


def test_abi_version_is_10_everywhere():
    from lofreq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    assert int(re.search(r"#define LFQ_ABI_VERSION (\d+)", hdr).group(1)) == 10
    assert _lib.LFQ_ABI_VERSION == 10
    assert _lib.load().lfq_abi_version() == 10


def test_release_library_still_reads_ten_environment_variables():
    def env_names(lib):
        data = open(os.path.join(ROOT, "lofreq_amd", lib), "rb").read()
        return {m.decode() for m in re.findall(rb"(?<![A-Z0-9_])((?:LFQ|LOCAL)_[A-Z0-9_]{3,})\x00", data)}
    knobs = {"LFQ_TIMING", "LFQ_SINGLE_STREAM", "LFQ_DEBUG_SYNC", "LFQ_PRIVATE_STREAM", "LFQ_SYNC_UPLOAD", "LFQ_BAQ_SCRATCH_MB",
             "LFQ_HOST_THREADS", "LFQ_HOST_LOOP_THREADS", "LFQ_HOST_SPIN_US", "LOCAL_WORLD_SIZE"}
    assert len(knobs) == 10
    assert env_names("liblofreq_amd.so") == knobs | {"LFQ_DEVICE", "LFQ_SLOT_DIR", "LOCAL_RANK"}
