"""CPU tests: oracle pieces against the reference's OWN objects (fet.c, multtest.c, utils.c compiled
unmodified into oracle/_ref/libref_parts.so by `make -C oracle ref`).  Their outputs on the seeded cases are stored in
tests/golden/ref_parts.npz (oracle/ref_vectors.py), so the comparisons run everywhere; where oracle/_ref is built, the
stored outputs are checked against the live objects as well."""
import ctypes as C

import numpy as np
import pytest

import ref_vectors as rv


@pytest.fixture(scope="module")
def stored():
    return rv.load()


def test_stored_vectors_equal_live_reference(oracle, stored):
    """tests/golden/ref_parts.npz is what the reference's objects compute on the cases of oracle/ref_vectors.py"""
    R = oracle.ref_parts()
    if R is None or not hasattr(R, "kpa_ext_glocal") or not hasattr(R, "binom"):
        pytest.skip("oracle/_ref not built (reference tree absent)")
    live = rv.compute(R)
    assert sorted(live) == sorted(stored)
    for k in live:
        assert np.array_equal(live[k], stored[k]), k


def test_fisher_exact_bitwise(oracle, stored):
    L = oracle.lib()
    for (a, b, c, d), want in zip(stored["fisher_in"], stored["fisher_out"]):
        o = [C.c_double() for _ in range(3)]
        q1 = L.orc_fisher_exact(int(a), int(b), int(c), int(d), *o)
        assert q1 == want[0] and all(x.value == y for x, y in zip(o, want[1:])), (a, b, c, d)
    assert len(stored["fisher_in"]) == 4000


def test_multtest_bitwise(oracle, stored):
    L = oracle.lib()
    dp = C.POINTER(C.c_double)
    ns = stored["mt_n"]
    ps = rv.split(stored["mt_p"], ns)
    bonf, holm = rv.split(stored["mt_bonf"], ns), rv.split(stored["mt_holm"], ns)
    fdr = rv.split(stored["mt_fdr_idx"], stored["mt_fdr_n"])
    for i, (n, alpha, p) in enumerate(zip(ns, stored["mt_alpha"], ps)):
        n = int(n)
        a = p.copy()
        L.orc_bonf_corr(a.ctypes.data_as(dp), n, 0)
        assert np.array_equal(a, bonf[i])
        a = p.copy()
        L.orc_holm_bonf_corr(a.ctypes.data_as(dp), n, alpha, 0)
        assert np.array_equal(a, holm[i])
        for j, ntests in enumerate((0, 2 * n)):
            rej = (C.c_long * n)()
            n1 = L.orc_fdr(p.ctypes.data_as(dp), n, alpha, ntests, rej)
            assert n1 == stored["mt_fdr_n"][2 * i + j]
            assert sorted(rej[k] for k in range(n1)) == fdr[2 * i + j].tolist()
    assert len(ns) == 20


def test_int_median_and_dbl_cmp(oracle, stored):
    L = oracle.lib()
    for v, want in zip(rv.split(stored["median_v"], stored["median_len"]), stored["median_out"]):
        v = np.ascontiguousarray(v, np.int32)
        assert L.orc_int_median(v.ctypes.data_as(C.POINTER(C.c_int)), len(v)) == want
    L.orc_dbl_cmp.argtypes = [C.c_void_p, C.c_void_p]
    for (x, y), want in zip(stored["dbl_cmp_in"], stored["dbl_cmp_out"]):
        a, b = C.c_double(x), C.c_double(y)
        assert L.orc_dbl_cmp(C.byref(a), C.byref(b)) == want
