"""The work items of the row-segment kernels (lofreq_amd/csrc/lfq_seg_items.h) on the host: lfq_seg_items_check.cpp, the
header's stand-alone program, is compiled with the host compiler and plays producers and consumer over class lists with
0, 1, 3, per_class and per_class + 1 records, n_seg in {2, 3, 8} and phase1 in {0, 1} mixed within a list, for both modes.

Asserted: every existing (class, record, segment) pair is an item exactly once, nothing else is, the items of a mode are
entries 0 .. n - 1 of its list (wavefront i runs item i: the live wavefronts are a prefix of the launch) and nothing is
written outside them, and the live pairs are the ones the rule these kernels had before -- item = record * LFQ_SEG_MAX +
r, skipped unless phase1 <= r < n_seg -- visits; where every record has LFQ_SEG_MAX new segments and the records arrive
class by class, the order is that rule's too."""
import itertools
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")
SEG_MAX, N_CLASSES, MODE0_CLASSES = 8, 5, 2
PER_CLASS = 5
COUNTS = (0, 1, 3, PER_CLASS, PER_CLASS + 1)
SHAPES = [(2, 0), (3, 1), (8, 0), (2, 1), (8, 1), (3, 0)]      # (n_seg, phase1)


def _compile(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp), name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                        "-I" + os.path.join(ROOT, "include")] + flags
                       + [os.path.join(CSRC, "lfq_seg_items_check.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe, r = _compile(tmp_path_factory.mktemp("segitems"), "lfq_seg_items_check", [])
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, scenarios):
    """scenarios: [(per_class, [(cls, n_seg, phase1), ...])] -> per scenario ({mode: (n, stray)}, {mode: [(cls, slot, r, rec)]})"""
    text = "".join("S %d %d\n%s" % (pc, len(recs), "".join("%d %d %d\n" % r for r in recs)) for pc, recs in scenarios)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out, heads, items = [], {}, {0: [], 1: []}
    for line in p.stdout.split("\n")[:-1]:
        f = line.split()
        if f[0] == "M":
            heads[int(f[1])] = (int(f[2]), int(f[3]))
        elif f[0] == "I":
            assert int(f[2]) == len(items[int(f[1])])           # items come in list order
            items[int(f[1])].append(tuple(int(x) for x in f[3:]))
        else:
            out.append((heads, items))
            heads, items = {}, {0: [], 1: []}
    assert len(out) == len(scenarios)
    return out


def _mode(cls):
    return 1 if cls >= MODE0_CLASSES else 0


def _kept(per_class, recs):
    """the records that get a slot, per class in arrival order: {cls: [(n_seg, phase1)]}"""
    lists = {c: [] for c in range(N_CLASSES)}
    for cls, n_seg, phase1 in recs:
        lists[cls].append((n_seg, phase1))
    return {c: l[:per_class] for c, l in lists.items()}


def _legacy_items(per_class, recs, mode):
    """the rule before the item lists: class-major, item = record * SEG_MAX + r, live where phase1 <= r < n_seg"""
    kept, live = _kept(per_class, recs), []
    for cls in range(N_CLASSES):
        if _mode(cls) != mode:
            continue
        for i in range(len(kept[cls]) * SEG_MAX):
            n_seg, phase1 = kept[cls][i // SEG_MAX]
            if phase1 <= i % SEG_MAX < n_seg:
                live.append((cls, i // SEG_MAX, i % SEG_MAX))
    return live


def _scenarios():
    rng = random.Random(20261020)
    out = []
    for a, b, c in itertools.product(COUNTS, repeat=3):
        counts = (a, b, c, a, b)
        order = [cls for cls in range(N_CLASSES) for _ in range(counts[cls])]
        rng.shuffle(order)
        out.append((PER_CLASS, [(cls,) + SHAPES[(i + a) % len(SHAPES)] for i, cls in enumerate(order)]))
    return out


def _check(exe):
    scen = _scenarios()
    n_items = 0
    for (pc, recs), (heads, items) in zip(scen, _run(exe, scen)):
        kept = _kept(pc, recs)
        for mode in (0, 1):
            exp = [(cls, slot, r) for cls in range(N_CLASSES) if _mode(cls) == mode
                   for slot, (n_seg, phase1) in enumerate(kept[cls]) for r in range(phase1, n_seg)]
            got = items[mode]
            assert heads[mode] == (len(exp), 0), (recs, mode, heads)        # a prefix, and nothing written beyond it
            assert all(rec == cls * pc + slot and slot < pc for cls, slot, r, rec in got)
            pairs = [g[:3] for g in got]
            assert len(set(pairs)) == len(pairs), ("an item twice", recs, mode)
            assert sorted(pairs) == sorted(exp), (recs, mode)
            assert sorted(pairs) == sorted(_legacy_items(pc, recs, mode)), (recs, mode)
            n_items += len(got)
    return n_items


def test_every_pair_once_and_dense(prog):
    """125 mixes of class counts 0, 1, 3, per_class, per_class + 1 with n_seg and phase1 mixed within each list"""
    assert _check(prog) > 2000


def test_full_records_keep_the_old_order(prog):
    """seg_max = 8 with nothing to skip (every record 8 new segments, records class by class): item i is the pair the
    stride rule gave it"""
    for counts in ((3, 1, 2, 0, PER_CLASS + 1), (0, 0, 0, 0, 1), (PER_CLASS, PER_CLASS, PER_CLASS, PER_CLASS, PER_CLASS)):
        recs = [(cls, SEG_MAX, 0) for cls in range(N_CLASSES) for _ in range(counts[cls])]
        (heads, items), = _run(prog, [(PER_CLASS, recs)])
        for mode in (0, 1):
            assert [g[:3] for g in items[mode]] == _legacy_items(PER_CLASS, recs, mode)


def test_empty_lists(prog):
    (heads, items), = _run(prog, [(PER_CLASS, [])])
    assert heads == {0: (0, 0), 1: (0, 0)} and items == {0: [], 1: []}


def test_sanitized_build_runs_clean(tmp_path):
    """the same program under the host compiler's address and undefined-behaviour sanitizers, over the whole table"""
    exe, r = _compile(tmp_path, "lfq_seg_items_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link a sanitized program: " + r.stderr[-300:])
    assert _check(exe) > 2000
