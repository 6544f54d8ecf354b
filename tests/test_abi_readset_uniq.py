"""CPU tests: the ABI of the read-level uniq -- lfq_readset_pileup_sites, lfq_readset_uniq and lfq_last_sites_times are declared,
bound and exported, NULL arguments are refused without a device, the three ABI numbers still agree at 10 and the release
library still reads its ten environment variables.  No compute."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_new_symbols_are_declared_bound_and_exported():
    from lofreq_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "lofreq_amd.h")).read()
    assert re.search(r"int lfq_readset_pileup_sites\(lfq_ctx \*ctx, lfq_readset \*rs, const int64_t \*site_pos, int64_t n_sites, "
                     r"int min_plp_bq,\s*lfq_tracks \*tracks_out, int32_t \*coverage_plp_out_or_null, "
                     r"int32_t \*num_tails_out_or_null\);", hdr)
    assert re.search(r"int lfq_readset_uniq\(lfq_ctx \*ctx, lfq_readset \*rs, const lfq_uniq_variants \*vars, int use_det_lim, "
                     r"int min_plp_bq,\s*lfq_uniq_result \*out\);", hdr)
    assert "int lfq_last_sites_times(lfq_ctx *ctx, lfq_sites_times *t);" in hdr
    for name in ("lfq_readset_pileup_sites", "lfq_readset_uniq", "lfq_last_sites_times"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    vp = C.c_void_p
    assert L.lfq_readset_pileup_sites.argtypes == [vp, vp, vp, C.c_int64, C.c_int, C.POINTER(_lib.Tracks), vp, vp]
    assert L.lfq_readset_uniq.argtypes == [vp, vp, C.POINTER(_lib.UniqVariants), C.c_int, C.c_int, C.POINTER(_lib.UniqResult)]
    assert L.lfq_last_sites_times.argtypes == [vp, C.POINTER(_lib.SitesTimes)]
    # the structs as the header lays them out
    assert C.sizeof(_lib.UniqVariants) == 8 * 8 and C.sizeof(_lib.UniqResult) == 5 * 8 and C.sizeof(_lib.SitesTimes) == 40
    from lofreq_amd import pileup
    assert callable(pileup.ReadSet.pileup_sites) and callable(pileup.ReadSet.uniq)


def test_null_arguments_are_refused_before_a_device_is_touched():
    from lofreq_amd import _lib
    L = _lib.load()
    t, v, o, st = _lib.Tracks(), _lib.UniqVariants(), _lib.UniqResult(), _lib.SitesTimes()
    assert L.lfq_readset_pileup_sites(None, None, None, 0, 3, None, None, None) == -1
    assert L.lfq_readset_pileup_sites(None, None, None, 0, 3, C.byref(t), None, None) == -1
    assert L.lfq_readset_uniq(None, None, None, 0, 3, None) == -1
    assert L.lfq_readset_uniq(None, None, C.byref(v), 0, 3, C.byref(o)) == -1
    assert L.lfq_readset_uniq(None, None, C.byref(v), 1, 3, None) == -1
    assert L.lfq_last_sites_times(None, C.byref(st)) == -1 and L.lfq_last_sites_times(None, None) == -1


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
