"""The bound gate of the screen kernel (lofreq_amd/csrc/lfq_bound.h) on the host: lfq_bound_check.cpp, the header's
stand-alone program, is compiled with the host compiler and run over a table of inputs; its B is set against the exact tail
(dp_edges.exact_log_tail) of a column that holds the counted rows at exactly p_lo plus other rows.

The property: B never exceeds that tail -- a larger B could drop a column the reference does not prune.  B is a partial sum
of the tail's non-negative terms computed with at most 2 K + J + 12 < 100 multiplications and additions of positive doubles
(1.1e-16 relative each), so "never exceeds" is asserted with a bar of 1e-12 in log B: a hundred times the rounding, a
millionth of the 1e-6 slack the kernel prunes with."""
import math
import os
import shutil
import subprocess

import pytest

import dp_edges as de

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")
LOG_BAR = 1e-12
QLO, SHIFT, CODES, SUBSET = 31, 6, 32, 2048
KS = range(1, 32)
EXTRA_QS = (2, 31, 32, 41)
N_EXTRA = 3


def _compile(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp), name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I" + CSRC,
                        "-I" + os.path.join(ROOT, "include")] + flags
                       + [os.path.join(CSRC, "lfq_bound_check.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe, r = _compile(tmp_path_factory.mktemp("bound"), "lfq_bound_check", [])
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, lines):
    r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return out


def _n_los(k):
    return (0, k - 1, k, k + 1, SUBSET)


def _table(q_rows):
    """(K, n_lo, extra quality or None) for every K, every n_lo of the issue's list, without and with N_EXTRA other rows"""
    return [(k, n, xq) for k in KS for n in _n_los(k) for xq in (None,) + EXTRA_QS]


def _check_rows(exe, q_rows, p_lo):
    """the counted rows have quality q_rows in the exact column, the gate is told p_lo; -> (rows with B > 0, worst log excess)"""
    rows = _table(q_rows)
    out = _run(exe, ["T %s %d %d" % (float(p_lo).hex(), n, k) for k, n, _ in rows])
    fired, worst, cache = 0, -math.inf, {}
    for (k, n_lo, xq), o in zip(rows, out):
        code, m, b = int(o.split()[0]), int(o.split()[1]), float(o.split()[2])
        assert code == min(n_lo >> SHIFT, CODES - 1) and m == code << SHIFT and m <= n_lo
        if m < k:
            assert b == 0.0, (k, n_lo, m, b)        # fewer counted rows than alt bases: no statement
            continue
        assert 0.0 < b <= 1.0 + 1e-12, (k, n_lo, b)
        fired += 1
        # the exact column: n_lo rows at q_rows (the kernel only knows m <= n_lo of them) and, with xq, three more rows
        spec = dict(n=n_lo + (N_EXTRA if xq is not None else 0), q=q_rows, q2=xq, n_q2=N_EXTRA if xq is not None else 0)
        key = (k, spec["n"], xq)
        if key not in cache:
            cache[key] = de.exact_log_tail(k, spec)
        excess = math.log(b) - cache[key]
        worst = max(worst, excess)
        assert excess <= LOG_BAR, ("false prune possible", k, n_lo, m, xq, b, cache[key])
    return fired, worst


def test_bound_never_above_exact_tail(prog):
    """K = 1..31 x n_lo = 0, K - 1, K, K + 1, 2048, the counted rows at Q31 = p_lo, alone and with three rows of Q2 / Q31 /
    Q32 / Q41 beside them"""
    fired, worst = _check_rows(prog, QLO, de.lut_p(QLO))
    print("\nbound gate: %d rows with B > 0, largest log B - log exact tail %.3g" % (fired, worst))
    assert fired >= 5 * len(KS)                     # n_lo = 2048 says something for every K


def test_bound_has_power(prog):
    """not a soundness property but the point of the gate: with 1984 rows at Q31 the J + 1 terms B keeps are most of
    P(Bin(m, p_lo) >= K) (mean 1.57: for K = 1 the terms 1..4 are 0.77 of 0.79, for larger K more), and at the benchmark's
    Bonferroni factor and significance level (3e6, 0.01) every column with K <= 8 is dropped"""
    p = de.lut_p(QLO)
    out = _run(prog, ["T %s %d %d" % (float(p).hex(), SUBSET, k) for k in KS])
    for k, o in zip(KS, out):
        b = float(o.split()[2])
        exact = de.exact_log_tail(k, dict(n=(CODES - 1) << SHIFT, q=QLO))
        assert math.log(b) >= exact + math.log(0.9), (k, b, exact)
        if k <= 8:
            assert b * 3e6 > 0.01, (k, b)


def test_quantisation_rounds_down(prog):
    """every n_lo of the subset: the rows the gate assumes are never more than the rows counted, and at most 63 fewer"""
    p = de.lut_p(QLO)
    ns = list(range(0, SUBSET + 1)) + [SUBSET + 1, 4096, 2 ** 31 - 1, 2 ** 32 - 1]
    out = _run(prog, ["T %s %d 1" % (float(p).hex(), n) for n in ns])
    for n, o in zip(ns, out):
        code, m = int(o.split()[0]), int(o.split()[1])
        assert 0 <= code < CODES and m == code << SHIFT and m <= n
        assert n - m < (1 << SHIFT) or code == CODES - 1


def _lut_line(lo, hi, lut):
    return "L %d %d %d %s" % (lo, hi, len(lut), " ".join(float(v).hex() for v in lut))


def test_lut_edge(prog):
    """p_lo is the smallest entry over [lo, Q_lo] of the table it is given, monotone or not; no usable entry = gate off (0).
    With a table whose entry 20 is the probability of Q50, rows of quality 20 are counted rows of p = 1e-5 = p_lo: the bound
    stays below their exact tail."""
    mono = [de.lut_p(q) for q in range(256)]
    dip = list(mono)
    dip[20] = de.lut_p(50)
    cases = [
        (6, QLO, mono, mono[QLO]),
        (0, QLO, mono, mono[QLO]),
        (QLO, QLO, mono, mono[QLO]),
        (QLO + 1, QLO, mono, 0.0),                  # thresholds above Q_lo: nothing is ever counted
        (6, QLO, dip, dip[20]),
        (20, QLO, dip, dip[20]),
        (21, QLO, dip, mono[QLO]),
        (6, QLO, [0.0 if q == 10 else v for q, v in enumerate(mono)], 0.0),     # an entry the bound cannot use
        (0, QLO, [1.0] * 256, 0.0),
        (6, QLO, mono[:20], mono[19]),              # (entries the caller did not give are ignored)
    ]
    out = _run(prog, [_lut_line(lo, hi, lut) for lo, hi, lut, _ in cases])
    for (lo, hi, _, exp), o in zip(cases, out):
        assert float(o) == exp, (lo, hi, o, exp)
    fired, worst = _check_rows(prog, 50, dip[20])
    assert fired > 0
    # p_lo outside (0, 1): the program answers like the host, gate off
    assert _run(prog, ["T 0x0p+0 2048 3", "T 0x1p+0 2048 3"]) == ["0 0 0", "0 0 0"]


def test_sanitized_build_runs_clean(tmp_path):
    """the same program under the host compiler's address and undefined-behaviour sanitizers, over the whole table"""
    exe, r = _compile(tmp_path, "lfq_bound_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link a sanitized program: " + r.stderr[-300:])
    fired, _ = _check_rows(exe, QLO, de.lut_p(QLO))
    assert fired > 0
