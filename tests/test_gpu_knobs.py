"""-m gpu: the code paths that only run under an environment knob get the parity tests of their area, each in a process of
its own with the knob set -- so that nothing that can be selected at run time is untested.  Every knob here forces a path the
release library takes by itself for some input (no pool space, K >= 32, unsorted reads, wide bands, shallow / deep launch
shapes, a context with LFQ_GATE_NONE); the measured-and-rejected A/B variants that no input could reach -- other workgroup
shapes of the count kernels, LDS padding, the stream plan of round 4 -- are deleted with their knobs (profiles/NOTES.md).  The
two-workgroups-per-CU launch of the shared-wavefront count kernel, which an ungated context makes, is covered where it
happens: test_gpu_stability.py::test_submit_collect_dense_counts_without_strands.  The knobs are read once per process
(lfq_knobs(), lfq_internal.h); DESIGN.md section 7 says which build reads which.

Round 6: the release library reads ten variables, none of which changes a result; every other knob exists only in the tuning
build lofreq_amd/liblofreq_amd_tune.so (the same objects, lfq_host.cpp compiled under -DLFQ_TUNE), which the child processes
here load through LFQ_AMD_LIB.  test_release_library_ignores_the_tuning_knobs holds the release library to that."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

TUNE_LIB = os.path.join(ROOT, "lofreq_amd", "liblofreq_amd_tune.so")

DP = ["tests/test_gpu_parity.py", "-k", "default_conf_random or row_split or ragged_deep or underflow or fe_clamp or cells_below or "
      "golden_reference or dynamic_bonferroni or edge_cases"]
BAQ = ["tests/test_gpu_baq.py"]
PLP = ["tests/test_gpu_pileup.py", "tests/test_gpu_plpindel.py", "-k", "not host_loops and not window_search"]
CHAIN = ["tests/test_gpu_plpindel.py", "-k", "chain or device_only or device_packing", "tests/test_gpu_indel.py"]
# ... and the indel boundary rows (-k holds for every file of a run: the module's name selects its tests)
HOST_PACK = ["tests/test_gpu_plpindel.py", "-k", "chain or device_only or device_packing or test_gpu_indel_edges", "tests/test_gpu_indel.py",
             "tests/test_gpu_indel_edges.py"]

CASES = [
    ("LFQ_SPLIT_POOL_CELLS=0", DP),          # no row split: every long column on the unsplit kernels
    ("LFQ_SPLIT_POOL_CELLS=60000", DP),      # a pool that runs out: split and unsplit columns in one batch
    ("LFQ_LIGHT_KERNEL=wave", DP),           # one light column per wavefront (what K >= 32 gets anyway)
    ("LFQ_SCREEN_ROUNDS=2", DP),             # nearly every light column through the retry kernel
    ("LFQ_SINGLE_STREAM=1", DP),             # every kernel on one stream (what the counter passes run)
    ("LFQ_NO_SB_PRECOMPUTE=1", DP),          # strand bias computed at collect time only
    ("LFQ_COUNT_MULTI_BELOW=0", DP),         # shallow batches on the one-column-per-wavefront count kernel
    ("LFQ_COUNT_LPG4_BELOW=100000", DP),     # shared-wavefront count kernel: four lanes per column whatever the depth
    ("LFQ_COUNT_LPG8_BELOW=100000", DP),     # ... eight (and four for the shallowest batches)
    ("LFQ_COUNT_LPG4_BELOW=0", DP),          # ... never four
    ("LFQ_SEG_MAX=2", DP),                   # a big column in two row segments, a mid-class column in one piece after its first stretch (what a context with LFQ_GATE_NONE runs)
    ("LFQ_SEG_MAX_MID=3 LFQ_SEG_MAX_BIG=4", DP),   # ... other segment counts per class
    ("LFQ_BIG_ON_SIDE=1", DP),               # the unsplit big columns behind the big chain (what a context with LFQ_GATE_NONE runs)
    ("LFQ_PRIVATE_STREAM=1", DP),            # every context with a launch stream of its own (lfq_set_private_stream) ...
    ("LFQ_PRIVATE_STREAM=1", CHAIN),         # ... on the read-set chain as well
    ("LFQ_PILEUP_TILES=0", PLP),             # a wavefront per position instead of tiles of 64 positions
    ("LFQ_BAQ_ONE_VARIANT=1", BAQ),          # every wavefront through the register kernel's instantiation with the N case
    ("LFQ_BAQ_LDS=0", BAQ),                  # every read through the all-HBM BAQ kernel (what wide bands get)
    ("LFQ_PILEUP_ATOMIC=1", PLP),            # read-major pileup kernels (what unsorted reads get)
    ("LFQ_INDEL_HOST_PACK=1", HOST_PACK),    # indel pseudo-columns packed on the host
    ("LFQ_SYNC_UPLOAD=1", CHAIN),            # lfq_readset_create waits for its copies itself
    ("LFQ_HOST_SPIN_US=-1", CHAIN),          # host loops on threads created per loop
]


@pytest.mark.parametrize("knob,sel", CASES, ids=[c[0] for c in CASES])
def test_knob_selected_paths(knob, sel):
    env = dict(os.environ, LFQ_AMD_LIB=TUNE_LIB, **dict(kv.split("=") for kv in knob.split()))
    p = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"] + sel, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=800)
    tail = (p.stdout + p.stderr)[-1500:]
    assert p.returncode == 0, tail
    assert " passed" in p.stdout and "failed" not in p.stdout.splitlines()[-1], tail


EDGES = ["tests/test_gpu_dp_edges.py"]
EDGE_CASES = [
    ("LFQ_SPLIT_POOL_CELLS=0", EDGES),       # every big column on the unsplit big kernel, every mid column unsplit
    ("LFQ_SEG_MAX=2", EDGES),                # two row segments per split column
    ("LFQ_LIGHT_KERNEL=wave", EDGES + ["-k", "not screen_variant"]),    # no screen kernel (nothing to count retries of)
    ("LFQ_SCREEN_ROUNDS=2", EDGES),          # screen survivors after two windows to the retry kernel
    ("LFQ_BIG_ON_SIDE=1", EDGES),            # the unsplit big columns behind the big chain
]


@pytest.mark.parametrize("knob,sel", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_knob_selected_dp_edges(knob, sel):
    """the DP boundary tests (K, depth and pruning edges of every route) under the fallback knobs"""
    test_knob_selected_paths(knob, sel)


PLP_EDGES = ["tests/test_gpu_pileup_edges.py"]
PLP_EDGE_CASES = [
    ("LFQ_PILEUP_TILES=0", PLP_EDGES),       # a wavefront per position: the kernels the tile kernels must agree with
    ("LFQ_PILEUP_ATOMIC=1", PLP_EDGES),      # read-major pileup kernels
]


@pytest.mark.parametrize("knob,sel", PLP_EDGE_CASES, ids=[c[0] for c in PLP_EDGE_CASES])
def test_knob_selected_pileup_edges(knob, sel):
    """the pileup boundary rows (row capacity, rounds, tile and region edges) on the kernels that replace the tile kernels"""
    test_knob_selected_paths(knob, sel)


_SKIP_PROBE = r"""
import sys
sys.path.insert(0, "tests")
import numpy as np
import lofreq_amd as la
import util
caller = la.SnvCaller(0)
host = util.random_batch(np.random.default_rng(5), 64, 800, 1500, planted={c: 0.3 for c in range(0, 64, 2)})
recs, _, st = caller.call_snvs(util.to_pileup_batch(la, host), la.VarcallConf())
print("RECS", len(recs))
"""


def test_release_library_ignores_the_tuning_knobs():
    """LFQ_DEBUG_SKIP drops DP classes -- i.e. calls -- in the tuning build and must do nothing in the release library"""
    out = {}
    for name, lib in (("release", None), ("tune", TUNE_LIB)):
        env = dict(os.environ, LFQ_DEBUG_SKIP="light,mid,big")
        env.pop("LFQ_AMD_LIB", None)
        if lib:
            env["LFQ_AMD_LIB"] = lib
        p = subprocess.run([sys.executable, "-c", _SKIP_PROBE], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-1500:]
        out[name] = int(p.stdout.split("RECS")[1])
    env = dict(os.environ)
    env.pop("LFQ_AMD_LIB", None)
    p = subprocess.run([sys.executable, "-c", _SKIP_PROBE], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    plain = int(p.stdout.split("RECS")[1])
    assert plain >= 20 and out["release"] == plain and out["tune"] < plain, (plain, out)
