#!/usr/bin/env python
"""Stored outputs of the reference's own objects (oracle/_ref/libref_parts.so: fet.c, multtest.c, utils.c, kprobaln_ext.c,
binom.c + cdflib90, compiled unmodified) on the seeded cases of tests/test_ref_parts.py, tests/test_baq.py and
tests/test_uniq.py.  Those tests compare the restatement with tests/golden/ref_parts.npz, so they run where the reference
tree is absent; where oracle/_ref is built, tests/test_ref_parts.py also checks the file against the live objects.

    python oracle/ref_vectors.py        rewrites tests/golden/ref_parts.npz (needs oracle/_ref)

TEST INFRASTRUCTURE ONLY, like pyoracle.py.  Every array of the file is a flat concatenation; `*_len` / `*_n` give the
pieces."""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
import pyoracle  # noqa: E402

GOLDEN = os.path.join(_HERE, "..", "tests", "golden", "ref_parts.npz")
KPA_PARAMS = ((0.00001, 0.4), (0.001, 0.1), (0.1, 0.4))      # illumina, samtools' default, pacbio (kprobaln_ext.c:48-51)
KPA_SEEDS = range(6)


# ---- the seeded cases ---------------------------------------------------------------------------------------------------

def fisher_cases():
    rng = np.random.default_rng(0)
    out = []
    for i in range(4000):
        hi = 30 if i % 3 == 0 else 6000
        out.append([int(x) for x in rng.integers(0, hi, 4)])
    return np.array(out, np.int64)


def multtest_cases():
    """-> [(n, alpha, p)]; p rounded to 4 digits: ties on purpose"""
    rng = np.random.default_rng(1)
    return [(n, alpha, np.round(rng.random(n) ** 3, 4)) for n in (1, 2, 10, 50, 333) for alpha in (0.001, 0.05, 0.25, 1.0)]


def median_cases():
    rng = np.random.default_rng(2)
    return [rng.integers(0, 42, n).astype(np.int32) for n in (1, 2, 3, 10, 11, 100)]


DBL_CMP_CASES = [(1.0, 1.0 + 1e-16), (1.0, 1.0 + 3e-16), (0.5, 0.25), (1e-20, 2e-20)]


def kpa_random_read(rng, lq, indel=0, n_frac=0.02):
    """a read of length lq against a reference window; `indel` = reference minus query length"""
    lr = lq + indel + int(rng.integers(0, 8))
    ref = rng.integers(0, 4, lr).astype(np.uint8)
    start = int(rng.integers(0, max(lr - lq - indel, 0) + 1))
    if indel >= 0:
        src = np.concatenate([ref[start:start + lq // 2], ref[start + lq // 2 + indel:start + lq + indel]])
    else:
        src = np.concatenate([ref[start:start + lq // 2], rng.integers(0, 4, -indel).astype(np.uint8),
                              ref[start + lq // 2:start + lq + indel]])
    query = src[:lq].copy()
    if len(query) < lq:
        query = np.concatenate([query, rng.integers(0, 4, lq - len(query)).astype(np.uint8)])
    mism = rng.random(lq) < 0.03
    query[mism] = (query[mism] + rng.integers(1, 4, int(mism.sum()))) % 4
    query[rng.random(lq) < n_frac] = 4
    ref[rng.random(lr) < n_frac / 2] = 4
    qual = np.clip(np.round(rng.normal(32, 8, lq)), 0, 60).astype(np.uint8)
    return ref, query, qual


def kpa_cases(seed):
    """-> [(ref, query, qual, bw)]: 60 reads of one seed"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(60):
        lq = int(rng.integers(1, 160))
        indel = int(rng.choice([0, 0, 0, 1, 3, -2, 12, -9]))
        if lq + indel < 1:
            indel = 0
        ref, query, qual = kpa_random_read(rng, lq, indel)
        bw = 7 if abs(len(ref) - lq) <= 7 else abs(len(ref) - lq) + 3
        out.append((ref, query, qual, bw))
    return out


def binom_cases():
    """-> [(n, k, af)]: edge cases, then ~6000 seeded ones around and away from the mean"""
    rng = np.random.default_rng(2024)
    cases = [(1, 0, 0.5), (1, 1, 0.5), (10, 0, 0.0), (10, 3, 1.0), (10, 10, 0.3), (370, 0, 0.95), (10000, 100, 0.5),
             (10000, 3108, 0.5), (10000, 3107, 0.5), (100000, 49000, 0.5), (100000, 50, 0.001), (5, -1, 0.5), (5, 6, 0.5),
             (0, 0, 0.5), (-3, 0, 0.5), (7, 2, -0.1), (7, 2, 1.5)]
    afs = [0.001, 0.004, 0.01, 0.02, 0.05, 0.08, 0.15, 0.3, 0.5, 0.6, 0.95, 0.999]
    for _ in range(6000):
        n = int(rng.choice([5, 30, 100, 400, 1500, 10000, 60000]) * rng.uniform(0.5, 1.5)) + 1
        af = float(rng.choice(afs))
        mode = rng.integers(0, 4)
        if mode == 0:
            k = int(rng.integers(0, n + 1))
        elif mode == 1:
            k = int(min(n, max(0, rng.normal(n * af, 3 * np.sqrt(n * af * (1 - af)) + 1))))
        elif mode == 2:
            k = int(rng.integers(0, max(1, int(n * af / 4)) + 1))
        else:
            k = int(min(n, n * af * rng.uniform(0.2, 1.2)))
        cases.append((n, k, af))
    return cases


# ---- the reference's outputs on them ------------------------------------------------------------------------------------

def compute(R):
    """the reference objects `R` (pyoracle.ref_parts()) on every case -> the arrays of tests/golden/ref_parts.npz"""
    dp = C.POINTER(C.c_double)
    out = {}
    fc = fisher_cases()
    fo = np.zeros((len(fc), 4))
    for i, (a, b, c, d) in enumerate(fc):
        r = [C.c_double() for _ in range(3)]
        fo[i, 0] = R.kt_fisher_exact(int(a), int(b), int(c), int(d), *r)
        fo[i, 1:] = [x.value for x in r]
    out.update(fisher_in=fc, fisher_out=fo)

    mc = multtest_cases()
    bonf, holm, fdr_idx, fdr_n = [], [], [], []
    for n, alpha, p in mc:
        b = p.copy()
        R.bonf_corr(b.ctypes.data_as(dp), n, 0)
        h = p.copy()
        R.holm_bonf_corr(h.ctypes.data_as(dp), n, alpha, 0)
        bonf.append(b)
        holm.append(h)
        for ntests in (0, 2 * n):
            ptr = C.POINTER(C.c_long)()
            k = R.fdr(p.ctypes.data_as(dp), n, alpha, ntests, C.byref(ptr))
            fdr_n.append(k)
            fdr_idx.append(np.sort(np.array([ptr[i] for i in range(k)], np.int64)))
    out.update(mt_n=np.array([m[0] for m in mc]), mt_alpha=np.array([m[1] for m in mc]),
               mt_p=np.concatenate([m[2] for m in mc]), mt_bonf=np.concatenate(bonf), mt_holm=np.concatenate(holm),
               mt_fdr_n=np.array(fdr_n, np.int64), mt_fdr_idx=np.concatenate(fdr_idx))

    med = median_cases()
    out.update(median_v=np.concatenate(med), median_len=np.array([len(v) for v in med]),
               median_out=np.array([R.int_median(v.ctypes.data_as(C.POINTER(C.c_int)), len(v)) for v in med]))
    cmp_out = []
    for x, y in DBL_CMP_CASES:
        a, b = C.c_double(x), C.c_double(y)
        cmp_out.append(R.dbl_cmp(C.byref(a), C.byref(b)))
    out.update(dbl_cmp_in=np.array(DBL_CMP_CASES), dbl_cmp_out=np.array(cmp_out))

    rows = {k: [] for k in ("seed", "bw", "lr", "lq", "ref", "query", "qual", "pr", "state", "q")}
    for seed in KPA_SEEDS:
        for ref, query, qual, bw in kpa_cases(seed):
            rows["seed"].append(seed)
            rows["bw"].append(bw)
            rows["lr"].append(len(ref))
            rows["lq"].append(len(query))
            rows["ref"].append(ref)
            rows["query"].append(query)
            rows["qual"].append(qual)
            for d, e in KPA_PARAMS:
                pr, state, q = pyoracle.kpa_glocal(ref, query, qual, d, e, bw, use_reference=True)
                rows["pr"].append(pr)
                rows["state"].append(state)
                rows["q"].append(q)
    for k in ("seed", "bw", "lr", "lq", "pr"):
        out["kpa_" + k] = np.array(rows[k], np.int64)
    for k in ("ref", "query", "qual", "state", "q"):
        out["kpa_" + k] = np.concatenate(rows[k])

    bc = binom_cases()
    bp, bs = [], []
    for n, k, af in bc:
        p, s = pyoracle.ref_binom(n, k, af)
        bp.append(p)
        bs.append(s)
    out.update(binom_in=np.array(bc, np.float64), binom_p=np.array(bp), binom_status=np.array(bs, np.int64))
    return out


def load():
    """tests/golden/ref_parts.npz as a dict of arrays"""
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def split(flat, lengths):
    """a flat concatenation -> its pieces"""
    return np.split(flat, np.cumsum(lengths)[:-1])


def kpa_by_seed(v, seed):
    """-> [(ref, query, qual, bw, [(d, e, pr, state, q) for KPA_PARAMS])] of one seed, from the stored arrays"""
    lr, lq = v["kpa_lr"], v["kpa_lq"]
    refs, queries, quals = split(v["kpa_ref"], lr), split(v["kpa_query"], lq), split(v["kpa_qual"], lq)
    np_ = len(KPA_PARAMS)
    states, qs = split(v["kpa_state"], np.repeat(lq, np_)), split(v["kpa_q"], np.repeat(lq, np_))
    out = []
    for i in np.flatnonzero(v["kpa_seed"] == seed):
        runs = [(d, e, int(v["kpa_pr"][np_ * i + j]), states[np_ * i + j], qs[np_ * i + j])
                for j, (d, e) in enumerate(KPA_PARAMS)]
        out.append((refs[i], queries[i], quals[i], int(v["kpa_bw"][i]), runs))
    return out


if __name__ == "__main__":
    R = pyoracle.ref_parts()
    if R is None or not hasattr(R, "kpa_ext_glocal") or not hasattr(R, "binom"):
        raise SystemExit("oracle/_ref/libref_parts.so is not built (make -C oracle ref, where the reference tree is mounted)")
    v = compute(R)
    np.savez_compressed(GOLDEN, **v)
    print("wrote %s (%d arrays, %d bytes)" % (os.path.normpath(GOLDEN), len(v), os.path.getsize(GOLDEN)))
