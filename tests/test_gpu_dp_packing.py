"""-m gpu: the launch shapes of the latency-bound long-column kernels (mid kernel, row-segment kernels) of a context that
queues its batches without a gate: 4, 8 or 16 wavefronts per workgroup, the items of the segment kernels listed densely
(lofreq_amd/csrc/lfq_seg_items.h, lfq_batch_device_impl).

Batches of dp_edges columns with 0, 1, 15, 16, 17 and 33 mid-class and as many big-class columns -- the workgroup edges of
16 wavefronts -- whose K cycles through the class edges 63/64, 252/253, 504/505 (and 1008/1009), each as deep as it has to be
to split (lfq_split_plan: eight chunks behind the mid class's first stretch, eight chunks of a big column), and one batch
that mixes K > LFQ_SPLIT_MAX_K (unsplit) with split columns.  Every batch is checked against the oracle and the exact tails
like test_gpu_dp_edges.py does, on a context with set_batch_gate("none"); and it runs in child processes on the tuning
build with LFQ_DP_WG_WAVES = 4 and 16 (a process reads its knobs once), under the segment bounds such a context chooses
and under LFQ_SEG_MAX_MID=3 LFQ_SEG_MAX_BIG=4 (records with a phase-1 stretch, 2 to 4 segments): records, counts and
dp_work must be the same bytes whatever the shape.  A context without set_batch_gate launches 4 wavefronts per
workgroup whatever the knob says: same bytes again."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import dp_edges as de
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNE_LIB = os.path.join(ROOT, "lofreq_amd", "liblofreq_amd_tune.so")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

NO_PRUNE = dict(sig=0.999, bonf_dynamic=0, bonf_subst=1)       # as test_gpu_dp_edges.py: every column runs all its rows
N_LONG = (0, 1, 15, 16, 17, 33)
MID_KS = (63, 64, 100, 249)                     # 1 / 4 cells per lane of the mid kernel and of segment classes 0 / 1
BIG_KS = (252, 253, 504, 505, 1008, 1009)       # segment classes 1 / 2 / 3 / 4 (K = 250..252: a big column in mode 0's list)
MIN_ROWS = 64 * (de.PHASE1 + 2 * de.C["LFQ_SEG_MIN_CHUNKS_SHORT"][0]) + 70      # splits behind the first stretch, odd tail
CHILD_KNOBS = {"w4": "LFQ_DP_WG_WAVES=4", "w16": "LFQ_DP_WG_WAVES=16",
               "w4_seg": "LFQ_DP_WG_WAVES=4 LFQ_SEG_MAX_MID=3 LFQ_SEG_MAX_BIG=4",
               "w16_seg": "LFQ_DP_WG_WAVES=16 LFQ_SEG_MAX_MID=3 LFQ_SEG_MAX_BIG=4"}
UNGATED = "17"                                  # the batch that also runs on a context without set_batch_gate


def _long_column(k, i):
    """K alt bases in max(4 K, MIN_ROWS) rows (K = 63: as few as keep it out of the light class) at the quality that puts
    the mean just below K: the column is neither pruned nor decided early, every row runs"""
    n = de.light_min_n(k) - 1 if k < de.MID_K else max(4 * k, MIN_ROWS) + i % 3
    q = max(de.MIN_BQ, int(math.ceil(-10.0 * math.log10(k / n))))
    col = de.edge_column(n, (k, 0, 0), q=q, alt_at=("first", "last", "spread")[i % 3])
    assert de.dp_class(k, n) == ("big" if k >= de.BIG_K else "mid"), (k, n)
    return col


def _batch(name):
    light = [de.edge_column(200, (3, 0, 0), q=30, alt_at="spread") for _ in range(3)]
    if name == "mixed":
        ks = [de.SPLIT_MAX_K + 1, 300, 100, de.SPLIT_MAX_K + 1, 505, 1009, 64]
        cols = [de.edge_column(8100, (k, 0, 0), q=6) if k > de.SPLIT_MAX_K else _long_column(k, i) for i, k in enumerate(ks)]
    else:
        n = int(name)
        cols = [_long_column(ks[i % len(ks)], i) for i in range(n) for ks in (MID_KS, BIG_KS)]
    return de.batch_of(light[:2] + cols + light[2:])


BATCHES = [str(n) for n in N_LONG] + ["mixed"]


def _result_bytes(recs, counts, work):
    recs = recs[np.lexsort((recs["alt"], recs["col"]))]
    return dict(recs=np.frombuffer(recs.tobytes(), np.uint8), counts=np.frombuffer(counts.tobytes(), np.uint8),
                work=np.array([work[k] for k in sorted(work)], np.int64))


def _run(la, host, gate):
    caller = la.SnvCaller(0)
    try:
        if gate:
            caller.set_batch_gate(gate)
        recs, counts, _ = caller.call_snvs(util.to_pileup_batch(la, host), la.VarcallConf(**NO_PRUNE), want_counts=True)
        return _result_bytes(recs, counts, caller.dp_work())
    finally:
        caller.close()


def child_main(out_dir):
    """in a child process (its knobs are in the environment): every batch on a fresh gate-"none" context, UNGATED also
    on a plain one; the results as <out_dir>/<batch>_<context>.npz"""
    import lofreq_amd as la
    for name in BATCHES:
        host = _batch(name)
        for ctx, gate in (("none", "none"),) + ((("plain", None),) if name == UNGATED else ()):
            np.savez(os.path.join(out_dir, "%s_%s.npz" % (name, ctx)), **_run(la, host, gate))


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """{knobs: directory of that child's results}: one process per shape and segment bound, all batches in it"""
    out = {}
    for key, knobs in CHILD_KNOBS.items():
        d = str(tmp_path_factory.mktemp("packing_" + key))
        env = dict(os.environ, LFQ_AMD_LIB=TUNE_LIB, **dict(kv.split("=") for kv in knobs.split()))
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_dp_packing as t; t.child_main(%r)" % (
            ROOT, os.path.join(ROOT, "tests"), d)
        p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=250)
        assert p.returncode == 0, (knobs, (p.stdout + p.stderr)[-2000:])
        out[key] = d
    return out


def _load(d, name, ctx):
    with np.load(os.path.join(d, "%s_%s.npz" % (name, ctx))) as z:
        return {k: z[k] for k in z.files}


def _same(a, b, what):
    for k in ("recs", "counts", "work"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("name", BATCHES)
def test_packed_shapes_match_oracle_and_each_other(oracle, children, name):
    import lofreq_amd as la
    from test_gpu_dp_edges import _check_run
    host = _batch(name)
    ores, oconf = util.run_oracle(oracle, host, **NO_PRUNE)
    routes = ["packing"] * len(host["specs"])
    caller = la.SnvCaller(0)
    try:
        caller.set_batch_gate("none")
        conf = la.VarcallConf(**NO_PRUNE)
        recs, counts, _ = caller.call_snvs(util.to_pileup_batch(la, host), conf, want_counts=True)
        here = _result_bytes(recs, counts, caller.dp_work())
        worst = {}
        recs, work, st = _check_run(la, caller, host, NO_PRUNE, ores, oconf, routes, worst)
    finally:
        caller.close()
    n_long = sum(de.dp_class(max(s["counts"]), s["n"]) in ("mid", "big") for s in host["specs"])
    assert work["n_mid"] + work["n_big"] == n_long and work["n_light"] == 3, work
    assert len(recs) >= n_long                  # every long column is called: its DP ran to the last row
    w4, w16 = _load(children["w4"], name, "none"), _load(children["w16"], name, "none")
    _same(w4, w16, "4 against 16 wavefronts per workgroup")
    _same(here, w4, "this process against the tuning build")
    _same(_load(children["w4_seg"], name, "none"), _load(children["w16_seg"], name, "none"), "4 against 16, three / four segments")
    print("\npacking %s: %d long columns, %d records, max |dlog p| against the exact tail %.3g" % (
        name, n_long, len(recs), worst.get("packing", 0.0)))


def test_ungated_context_keeps_its_shape(children):
    """without set_batch_gate the knob selects nothing: the same bytes under 4 and 16, and in this process"""
    import lofreq_amd as la
    here = _run(la, _batch(UNGATED), None)
    for a, b in (("w4", "w16"), ("w4_seg", "w16_seg")):
        _same(_load(children[a], UNGATED, "plain"), _load(children[b], UNGATED, "plain"), (a, b))
    _same(here, _load(children["w4"], UNGATED, "plain"), "this process against the tuning build")
