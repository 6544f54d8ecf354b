"""The bound gate's decision as the scan makes it (lfq_bound_drops, lofreq_amd/csrc/lfq_bound.h) on the host: the header's
stand-alone program lfq_bound_check.cpp, compiled with the host compiler as tests/test_bound_gate.py does, answers the `D`
request for every n_lo code, K = 1..33, the MAXK of three screen variants and four Bonferroni factors.

Two properties:
  - it is the screen kernel's expression and nothing else: code != 0, K <= MAXK, lfq_bound_tail(code, K) * bonf > sig_s, with
    lfq_bound_tail taken from the program's own `T` answer and the product and comparison done here in the same doubles;
  - it never drops a column the reference keeps: the smallest exact tail a column with that code can have -- m = 64 * code
    rows of p_lo and nothing else, dp_edges.exact_log_tail, the tails test_bound_gate.py uses -- times the factor is above
    sig for every dropped combination (bar: 1e-12 in the logarithm, as there)."""
import math

import numpy as np
import pytest

import dp_edges as de
from test_bound_gate import CODES, LOG_BAR, QLO, SHIFT, _compile, _run

MAXKS = (5, 9, 31)
FACTORS = (1.0, 3.0, 90.0, 3e6)
KS = range(1, 34)
SIG = float(np.float32(0.01))               # LfqParams::sig: (double)(float)conf->sig
SIG_S = SIG * (1.0 + 1e-6)                  # ... * (1 + prune_slack)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe, r = _compile(tmp_path_factory.mktemp("scan_gate"), "lfq_bound_check", [])
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def answers(prog):
    """-> {(code, K, maxk, bonf): dropped}, {(code, K): B}"""
    p = float(de.lut_p(QLO)).hex()
    keys = [(c, k, mk, b) for c in range(CODES) for k in KS for mk in MAXKS for b in FACTORS]
    out = _run(prog, ["D %s %d %d %d %s %s" % (p, c, k, mk, float(b).hex(), float(SIG_S).hex()) for c, k, mk, b in keys])
    assert set(out) <= {"0", "1"}
    tails = [(c, k) for c in range(CODES) for k in KS]
    tout = _run(prog, ["T %s %d %d" % (p, c << SHIFT, k) for c, k in tails])
    for (c, _), o in zip(tails, tout):
        assert int(o.split()[0]) == c
    return {key: o == "1" for key, o in zip(keys, out)}, {ck: float(o.split()[2]) for ck, o in zip(tails, tout)}


def test_decision_is_the_screen_kernels_expression(answers):
    dropped, tail = answers
    n = 0
    for (c, k, mk, b), got in dropped.items():
        exp = c != 0 and k <= mk and tail[(c, k)] * b > SIG_S
        assert got == exp, (c, k, mk, b, tail[(c, k)], got)
        n += got
    # the table says something: drops at every factor, and none for a code of 0, K > MAXK or K beyond the widest variant
    assert n > 0 and all(any(g for (c, k, mk, b), g in dropped.items() if b == f) for f in FACTORS)
    assert not any(g for (c, k, mk, b), g in dropped.items() if c == 0 or k > mk or k > 31)
    assert any(g for (c, k, mk, b), g in dropped.items() if mk == 31 and k > 9)
    print("\nscan gate: %d of %d combinations dropped" % (n, len(dropped)))


def test_never_drops_what_the_reference_keeps(answers):
    dropped, _ = answers
    cache, worst = {}, math.inf
    for (c, k, mk, b), got in dropped.items():
        if not got:
            continue
        if (c, k) not in cache:
            cache[(c, k)] = de.exact_log_tail(k, dict(n=c << SHIFT, q=QLO))
        margin = cache[(c, k)] + math.log(b) - math.log(SIG)
        worst = min(worst, margin)
        assert margin > -LOG_BAR, ("dropped, but exact tail * factor <= sig", c, k, mk, b, cache[(c, k)])
    assert cache
    print("\nscan gate: %d exact tails, smallest log(tail * factor / sig) among dropped columns %.3g" % (len(cache), worst))
