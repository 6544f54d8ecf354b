"""The host half of the indel pileup (lofreq_amd/csrc/lfq_plp_indel_host.h) without a GPU: lfq_plp_indel_host_check.cpp, the
header's stand-alone program, is compiled with the host compiler and runs the stages -- events from the CIGARs, their merge,
the event tables part by part, the columns from the nine per-position counters, ev_off, the consensus flags, rd_aq, publish
-- serially, with the numbers of parts the input forces.  The counters, the kernel's share, are input: derived here from the
same CIGARs with min_plp_idq = 0, where every pileup entry passes and they are pure geometry (golden_util.py_indel_pileup,
itself pinned against the reference binary's dump by test_plpindel_restatement.py).

Asserted: on the golden fixtures the event tables and consensus flags are the reference binary's (the comparison
test_gpu_plpindel.py makes on the device); on hand-made reads built to hit the cuts the output is the same text for 1, 2, 3
and 5 parts and equals the restatement; the sanitized build runs the same cases clean."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lofreq_amd", "csrc")
OPS = "MIDNSHP=X"


def _compile(tmp, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp), name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                        "-I" + os.path.join(ROOT, "include")] + flags
                       + [os.path.join(CSRC, "lfq_plp_indel_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe, r = _compile(tmp_path_factory.mktemp("plpindelhost"), "lfq_plp_indel_host_check", [])
    assert r.returncode == 0, r.stderr
    return exe


def _kept(reads, keep):
    return [r for i, r in enumerate(reads) if keep is None or keep[i]]


def _case_text(reads, ref, begin, end, want, parts=(1, 1, 1), keep=None, all_columns=0, have_qsum=1, gather=0, idq=(0, 0, 0)):
    """one case of the program's input; `want` = py_indel_pileup of the kept reads (the counters come from it)"""
    has = [int(any(r.get(k) is not None for r in reads)) for k in ("bi", "bd", "ai", "ad", "sq")]
    out = ["%d %d %d %d 0  %d %d %d  %d %d %d  %d %d %d" % ((len(reads), len(ref), begin, end) + tuple(parts)
                                                          + (all_columns, have_qsum, gather) + tuple(idq)),
           " ".join(map(str, has + [int(keep is not None)])), ref or "-"]
    for i, r in enumerate(reads):
        m = len(r["seq"])
        fl = sum(b for b, k in ((1, "bi"), (2, "bd"), (4, "ai"), (8, "ad")) if r.get(k) is not None)
        tags = [(r[k] if r.get(k) is not None else np.zeros(m, np.uint8)) for k in ("bi", "bd", "ai", "ad")]
        assert all(len(t) == m for t in tags)
        out.append("%d %d %d %d %d %d %d %d" % (r["pos0"], r["mapq"], int(r["reverse"]), fl, -1 if r.get("sq") is None else r["sq"],
                                                1 if keep is None else keep[i], len(r["cigar"]), m))
        out.append(" ".join(str(l << 4 | OPS.index(op)) for op, l in r["cigar"]))
        for a in [r["seq"]] + tags:
            out.append(" ".join(map(str, np.asarray(a).tolist())))
    w = end - begin
    h = np.zeros((9, w), np.int64)
    ev_pos = set()
    for p, c in want.items():
        if begin <= p < end:
            h[:, p - begin] = [c["cov"], c["tails"], c["non_indels"], c["n_ins"], c["n_dels"], c["non_fw"][0], c["non_fw"][1],
                               sum(q for q, _ in c["ne"][0]), sum(q for q, _ in c["ne"][1])]
            if c["ev"][0] or c["ev"][1] or all_columns:
                ev_pos.add(p)
    out += [" ".join(map(str, row.tolist())) for row in h]
    if not have_qsum:                       # what the scatter pass would bring back: the non-event qualities, column by column
        for sd in range(2):
            q = [q for p in sorted(ev_pos) for q, _ in want[p]["ne"][sd]]
            out.append("%d %s" % (len(q), " ".join(map(str, q))))
    return "\n".join(out) + "\n"


def _run(exe, text):
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return p.stdout


def _parse(stdout):
    """-> per case dict(n=(ncols, ne0, ne1, events), cols={pos: fields}, ev={pos: ([...], [...])}, P=[...])"""
    cases, cur = [], dict(cols={}, ev={}, P=[])
    for line in stdout.split("\n")[:-1]:
        f = line.split()
        if f[0] == "N":
            cur["n"] = tuple(int(x) for x in f[1:])
        elif f[0] == "C":
            v = [int(x) for x in f[3:]]
            cur["cols"][int(f[1])] = dict(ref=f[2], cov=v[0], tails=v[1], non_indels=v[2], n_ins=v[3], n_dels=v[4], hrun=v[5],
                                          cons=v[6], non_fw=(v[7], v[12]), non_rv=(v[8], v[13]), ne=((v[9], v[10]), (v[14], v[15])))
        elif f[0] == "E":
            lists = [[int(x) for x in part.split()] for part in line.split(":")[1:]]
            cur["ev"].setdefault(int(f[1]), ([], []))[int(f[2])].append(dict(key=f[3], fw=int(f[4]), rv=int(f[5]), q=lists[0],
                                                                               aq=lists[1], mq=lists[2], sq=lists[3]))
        elif f[0] == "P":
            cur["P"].append(tuple(int(x) for x in f[1:]))
        else:
            assert f[0] == "END"
            cases.append(cur)
            cur = dict(cols={}, ev={}, P=[])
    return cases


def _cons(c):
    """plp.c:1231-1270 on a column of py_indel_pileup: some event's quality sum strictly above the side's non-event sum"""
    return int(any(max([0] + [sum(m[0] for m in ms) for ms in c["ev"][sd].values()]) > max(sum(q for q, _ in c["ne"][sd]), 0)
                   for sd in range(2)))


def _assert_equals_restatement(got, want, begin, end, all_columns=False):
    """every field the program printed against py_indel_pileup's columns -> the number of events compared"""
    assert sorted(got["cols"]) == sorted(p for p in want if begin <= p < end)
    n_ev, run = 0, [0, 0]
    for p in sorted(got["cols"]):
        g, w = got["cols"][p], want[p]
        assert (g["cov"], g["tails"], g["non_indels"], g["n_ins"], g["n_dels"]) == (w["cov"], w["tails"], w["non_indels"], w["n_ins"], w["n_dels"]), p
        assert g["non_fw"] == tuple(w["non_fw"]) and g["non_rv"] == tuple(w["non_rv"]), p
        assert g["cons"] == _cons(w), p
        with_arrays = bool(w["ev"][0] or w["ev"][1] or all_columns)
        for sd in range(2):
            assert g["ne"][sd] == (run[sd], run[sd] + (len(w["ne"][sd]) if with_arrays else 0)), (p, sd)
            run[sd] = g["ne"][sd][1]
            evs = got["ev"].get(p, ([], []))[sd]
            assert [e["key"] for e in evs] == list(w["ev"][sd].keys()), (p, sd)
            for e in evs:
                ms = w["ev"][sd][e["key"]]
                assert (e["q"], e["aq"], e["mq"]) == ([m[0] for m in ms], [m[1] for m in ms], [m[2] for m in ms]), (p, e["key"])
                assert e["sq"] == [min(m[3], 32767) for m in ms] and e["rv"] == sum(m[4] for m in ms) and e["fw"] == len(ms) - e["rv"]
                n_ev += 1
    return n_ev


# ---- the golden fixtures: what test_indel_columns_match_plpsummary compares on the device ----------------------------------

@pytest.mark.parametrize("parts", [(1, 1, 1), (3, 5, 2)], ids=lambda p: "parts%d%d%d" % p)
@pytest.mark.parametrize("name", ["plpindel_default.json", "plpindel_consindel.json"])
def test_golden_event_tables(prog, name, parts):
    fx, reads = gu.load_plpindel(os.path.join(gu.GOLDEN_DIR, name))
    ref = fx["genome"]
    want = gu.py_indel_pileup(reads, ref)
    got, = _parse(_run(prog, _case_text(reads, ref, 0, len(ref), want, parts=parts)))
    n_ev = 0
    for e in fx["columns"]:
        p = e["pos0"]
        c = got["cols"][p]
        assert c["ref"] == e["ref"] and c["hrun"] == e["hrun"], p
        assert bool(c["cons"]) == (e["cons"][0] in "+-"), (p, e["cons"])        # plp.c:1236-1270
        for sd, sn in enumerate(("ins", "dels")):
            E = e[sn]
            assert (c["non_fw"][sd], c["non_rv"][sd]) == (E["non_fw"], E["non_rv"]), (p, sn)
            evs = got["ev"].get(p, ([], []))[sd]
            assert [g["key"] for g in evs] == [ev["key"] for ev in E["events"]], (p, sn)
            for g, ev in zip(evs, E["events"]):
                assert (g["fw"], g["rv"]) == (ev["fw"], ev["rv"]), (p, ev["key"])
                for k, wv in (("q", gu.dec(ev["q"]).tolist()), ("aq", gu.dec(ev["aq"]).tolist()), ("mq", ev["mq"]),
                              ("sq", gu.dec(ev["sq"]).tolist())):
                    assert g[k] == wv, (p, ev["key"], k)
                n_ev += 1
    assert n_ev >= 20
    with_ev = {e["pos0"] for e in fx["columns"]}            # columns the binary printed no event for have none here either
    for p, c in got["cols"].items():
        if p not in with_ev:
            assert not c["cons"] and p not in got["ev"]
    assert got["n"][0] == len(got["cols"]) == sum(1 for p in want if want[p]["cov"] > 0)


# ---- hand-made reads at the cuts -----------------------------------------------------------------------------------------

_RNG = np.random.default_rng(20261020)
_G = _RNG.integers(0, 4, 300).astype(np.uint8)
_G[150:158] = 1                                             # a homopolymer for hrun
REF = "".join("ACGT"[c] for c in _G)
REF = REF[:40] + REF[40:60].lower() + REF[60:]               # (deletion keys are upper-cased)


def _read(pos, cigar, ins="", drop=0, tags="bi bd ai ad", sq=None, mapq=60, reverse=False):
    """a read whose bases match the reference; inserted bases from `ins`; `drop` bases fewer than the CIGAR asks for"""
    cig = gu.parse_cigar(cigar)
    seq, x, ins = [], pos, list(ins)
    for op, l in cig:
        if op in "M=X":
            seq += [int(_G[min(x + j, len(_G) - 1)]) for j in range(l)]
            x += l
        elif op in "DN":
            x += l
        elif op == "I":
            seq += [gu.SEQ_LETTERS.index(ins.pop(0)) if ins else int(_RNG.integers(0, 4)) for _ in range(l)]
        elif op == "S":
            seq += _RNG.integers(0, 4, l).tolist()
    seq = seq[:len(seq) - drop]
    r = {"pos0": pos, "cigar": cig, "seq": np.asarray(seq, np.uint8), "mapq": mapq, "reverse": reverse, "sq": sq}
    for k in ("bi", "bd", "ai", "ad"):
        r[k] = _RNG.integers(33 + 5, 33 + 60, len(seq)).astype(np.uint8) if k in tags.split() else None
    return r


def _cases():
    """name -> (reads sorted by position, begin, end, options, compare with the restatement?)"""
    c = {}
    # four events at 10, 20, 20, 30: the even cut of two parts (and the second of three) falls between the two at 20 and moves on
    c["cut_between_equal_positions"] = ([_read(0, "11M1I20M", ins="T"), _read(5, "16M2D20M", reverse=True), _read(6, "15M1I20M", ins="G"),
                                         _read(8, "23M3D10M")], 0, 80, {}, True)
    # read 0 (first scan part) has its event at 199, behind the events of the reads after it; reads 0 and 1 share that event
    c["event_behind_next_part"] = ([_read(0, "200M2D10M"), _read(5, "195M2D10M", reverse=True, mapq=30), _read(40, "10M1I30M", ins="A"),
                                    _read(45, "30M1D5M", tags="bi ai")], 0, 260, {}, True)
    # one event only: more parts than events, parts (and read ranges) without any
    c["one_event"] = ([_read(3, "30M"), _read(4, "10M2I10M", ins="CA", sq=7), _read(9, "25M", tags="")], 0, 60, {}, True)
    c["no_event"] = ([_read(3, "30M"), _read(9, "25M")], 0, 60, {}, True)
    # an insertion reached through a pad, a pad with nothing behind it, a pad followed by a match
    c["pads"] = ([_read(10, "10M1P2I10M", ins="GT"), _read(11, "9M1P10M"), _read(12, "12M1P"), _read(12, "8M1P1I1P1I5M", ins="AC")],
                 0, 60, {}, True)
    # events at the region's first and last position, and just outside on both sides
    c["region_edges"] = ([_read(5, "15M1I30M", ins="A"), _read(6, "15M1D30M"), _read(90, "30M2I20M", ins="TT"), _read(91, "30M1I20M", ins="C"),
                          _read(92, "28M3D20M")], 20, 120, {}, True)
    # an insertion whose bases run past the read's end: letter N (the restatement prints what is there: compared below by hand)
    c["insertion_past_read_end"] = ([_read(20, "10M3I", ins="GAT", drop=2), _read(21, "9M1I10M", ins="G")], 0, 60, {}, False)
    # a deletion running past ref_len, inside a region that does too
    c["deletion_past_ref_len"] = ([_read(270, "25M10D1M"), _read(280, "15M9D1M", reverse=True)], 250, 310, {}, True)
    # two keys at one column in order of first appearance (T, A, T again), ambiguity letters as they are
    c["two_keys_one_column"] = ([_read(30, "10M1I10M", ins="T"), _read(31, "9M1I10M", ins="A", reverse=True), _read(32, "8M1I10M", ins="T"),
                                 _read(33, "7M1I10M", ins="R", sq=49314), _read(34, "6M2D10M"), _read(35, "5M3D10M"), _read(36, "4M2D10M")],
                                0, 70, {}, True)
    # the -d cap drops read 1, the only one with the second key
    c["keep_mask"] = ([_read(30, "10M1I10M", ins="T"), _read(31, "9M1I10M", ins="A"), _read(32, "8M1I10M", ins="T")], 0, 70,
                      {"keep": [1, 0, 1]}, True)
    big = sorted([r for k in ("cut_between_equal_positions", "event_behind_next_part", "pads", "region_edges", "two_keys_one_column")
                  for r in c[k][0]], key=lambda r: r["pos0"])
    c["all_together"] = (big, 0, 300, {}, True)
    c["all_together_every_column"] = (big, 7, 231, {"all_columns": 1}, True)
    c["all_together_host_sums"] = (big, 0, 300, {"have_qsum": 0}, True)
    c["all_together_gathered"] = (big, 0, 300, {"gather": 1}, True)
    c["uniform_indelqual"] = (big, 0, 300, {"idq": (1, 33 + 45, 33 + 21)}, False)
    c["dindel_indelqual"] = (big, 0, 300, {"idq": (2, 0, 0)}, False)
    return c


PARTS = [(1, 1, 1), (2, 2, 2), (3, 3, 3), (5, 5, 5), (5, 1, 2), (1, 3, 5), (2, 5, 1)]


def _check_parts(exe):
    cases = _cases()
    names = sorted(cases)
    text, wants = [], {}
    for name in names:
        reads, begin, end, opt, _ = cases[name]
        wants[name] = gu.py_indel_pileup(_kept(reads, opt.get("keep")), REF)
        text += [_case_text(reads, REF, begin, end, wants[name], parts=p, **opt) for p in PARTS]
    blocks = _run(exe, "".join(text)).split("END\n")[:-1]
    assert len(blocks) == len(names) * len(PARTS)
    out, n_ev = {}, 0
    for i, name in enumerate(names):
        mine = blocks[i * len(PARTS):(i + 1) * len(PARTS)]
        for p, b in zip(PARTS, mine):
            assert b == mine[0], (name, p)
        out[name], = _parse(mine[0] + "END\n")
        reads, begin, end, opt, model = cases[name]
        if model:
            n_ev += _assert_equals_restatement(out[name], wants[name], begin, end, bool(opt.get("all_columns")))
    return out, n_ev


def test_parts_do_not_change_the_output(prog):
    out, n_ev = _check_parts(prog)
    assert n_ev > 60
    ev = lambda name, p, sd: [(e["key"], e["fw"], e["rv"]) for e in out[name]["ev"].get(p, ([], []))[sd]]
    # the cases are what they were built to be
    assert out["cut_between_equal_positions"]["n"][3] == 4 and sorted(out["cut_between_equal_positions"]["ev"]) == [10, 20, 30]
    assert ev("cut_between_equal_positions", 20, 0) == [("G", 1, 0)] and ev("cut_between_equal_positions", 20, 1) == [(REF[21:23].upper(), 0, 1)]
    assert ev("event_behind_next_part", 199, 1) == [(REF[200:202], 1, 1)] and sorted(out["event_behind_next_part"]["ev"]) == [49, 74, 199]
    assert out["event_behind_next_part"]["ev"][199][1][0]["mq"] == [60, 30]            # reads of one key in read order
    assert out["one_event"]["n"][3] == 1 and out["no_event"]["n"][3] == 0 and not out["no_event"]["ev"]
    assert out["one_event"]["ev"][13][0][0]["sq"] == [7]
    assert sorted(out["pads"]["ev"]) == [19] and ev("pads", 19, 0) == [("GT", 1, 0), ("AC", 1, 0)]
    assert sorted(out["region_edges"]["ev"]) == [20, 119]                               # 19 and 120 lie outside
    assert ev("insertion_past_read_end", 29, 0) == [("GNN", 1, 0), ("G", 1, 0)]
    assert ev("deletion_past_ref_len", 294, 1) == [(REF[295:300] + "NNNNN", 1, 0), (REF[295:300] + "NNNN", 0, 1)]
    assert [c["ref"] for p, c in sorted(out["deletion_past_ref_len"]["cols"].items()) if p >= 300] == ["N"] * 6    # 300 .. 305
    assert ev("two_keys_one_column", 39, 0) == [("T", 2, 0), ("A", 0, 1), ("R", 1, 0)]
    assert ev("two_keys_one_column", 39, 1) == [(REF[40:42].upper(), 2, 0), (REF[40:43].upper(), 1, 0)]
    assert out["two_keys_one_column"]["ev"][39][0][2]["sq"] == [32767]
    assert ev("keep_mask", 39, 0) == [("T", 2, 0)]
    # the consensus flags from the scattered qualities are the ones from the kernel's sums; gathered ai / ad are the host's
    for other in ("all_together_host_sums", "all_together_gathered"):
        assert out[other]["ev"] == out["all_together"]["ev"]
        assert {p: c["cons"] for p, c in out[other]["cols"].items()} == {p: c["cons"] for p, c in out["all_together"]["cols"].items()}
    assert any(c["cons"] for c in out["all_together"]["cols"].values()) and not all(c["cons"] for p, c in out["all_together"]["cols"].items()
                                                                                    if p in out["all_together"]["ev"])
    # every column gets its arrays: pos_off at every covered position of the region
    assert all((col >= 0) == (p in out["all_together_every_column"]["cols"]) for p, col, o0, o1 in out["all_together_every_column"]["P"])
    # computed indel qualities replace the tags: one value each (uniform), the stand-in's (Dindel)
    assert {q for es in out["uniform_indelqual"]["ev"].values() for e in es[0] for q in e["q"]} == {45}
    assert {q for es in out["uniform_indelqual"]["ev"].values() for e in es[1] for q in e["q"]} == {21}
    assert out["dindel_indelqual"]["n"] == out["all_together"]["n"]


def test_sanitized_build_runs_clean(tmp_path):
    """the same program under the host compiler's address and undefined-behaviour sanitizers, over the hand-made cases"""
    exe, r = _compile(tmp_path, "lfq_plp_indel_host_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link a sanitized program: " + r.stderr[-300:])
    assert _check_parts(exe)[1] > 60
