"""The case table of the sparse pileup and `lofreq uniq` on a read set (lfq_readset_pileup_sites, lfq_readset_uniq), shared
by tests/test_uniq_sites_cases.py (no GPU: the oracle road against plain restatements and against the binary's fixture) and
tests/test_gpu_readset_uniq.py (the device against the oracle road).  Every row says what it is there for.

The oracle road: oracle.pileup_region over the whole contig, picked at the variants' positions (columns, num_tails, event
tables), then orc_uniq_binom_batch / orc_uniq_detlim_batch and orc_uniq_mtc; the indel count goes through the oracle's
binomial as a column of `count` bases of the tested letter under the indel coverage."""
import functools
import json
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEQ_LETTERS = "ACGTN=MRSVWYHKDB"
CODE = {c: i for i, c in enumerate(SEQ_LETTERS)}


def uniq_filter(flag, mapq):
    """what uniq's mpileup keeps (lofreq_uniq.c:459-465 over mplp_func, plp.c:600-660): the default flag mask, no orphans,
    MAPQ in [1, 255]"""
    if flag & (4 | 256 | 512 | 1024):
        return False
    if (flag & 1) and not (flag & 2):
        return False
    return 1 <= mapq <= 255


def parse_cigar(s):
    return [(op, int(n)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", s)]


def make_ref(n, seed):
    return "".join(np.random.default_rng(seed).choice(list("ACGT"), n))


def rd(ref, pos0, cigar, qual=30, mapq=60, rev=False, ins="ACGTTGCA", sub=None):
    """a read as the product and the oracle take it: bases from the contig (upper-cased) with `sub` {reference position:
    letter} put in, inserted and clipped bases from `ins`; qual: one value or a list per query base"""
    seq, x, k = [], pos0, 0
    for op, l in parse_cigar(cigar):
        if op in "M=X":
            for j in range(l):
                b = (sub or {}).get(x + j, ref[x + j].upper() if x + j < len(ref) else "N")
                seq.append(CODE.get(b, 4))
            x += l
        elif op in "IS":
            for j in range(l):
                seq.append(CODE[ins[k % len(ins)]])
                k += 1
        elif op in "DN":
            x += l
    q = [qual] * len(seq) if np.isscalar(qual) else list(qual)
    assert len(q) == len(seq), (cigar, len(q), len(seq))
    return {"pos0": pos0, "cigar": parse_cigar(cigar), "seq": np.asarray(seq, np.uint8), "qual": np.asarray(q, np.uint8),
            "mapq": mapq, "reverse": bool(rev)}


def other(b, k=1):
    return "ACGT"[("ACGT".index(b.upper()) + k) % 4] if b.upper() in "ACGT" else "A"


def snv(ref, p, af=0.1, k=1, key=False):
    return (p, ref[p].upper(), other(ref[p], k), af, key)


def _case(name, why, ref, reads, variants, min_plp_bq=3):
    assert all(reads[i]["pos0"] <= reads[i + 1]["pos0"] for i in range(len(reads) - 1)), name
    return {"name": name, "why": why, "ref": ref, "reads": reads, "variants": variants, "min_plp_bq": min_plp_bq}


def _windows():
    ref = make_ref(700, 1)
    reads, var = [], [snv(ref, 5), snv(ref, 320)]
    for s, k in [(20, 1), (50, 63), (80, 64), (110, 65), (150, 128), (200, 129)]:
        for i in range(k):
            reads.append(rd(ref, s, "12M", qual=20 + i % 20, mapq=[60, 30, 255, 1][i % 4], rev=i % 2,
                            sub={s + 5: other(ref[s + 5])} if i % 3 == 0 else None))
        var.append(snv(ref, s + 5, af=[0.01, 0.2, 0.5][k % 3]))
    return _case("windows", "sites covered by exactly 0, 1, 63, 64, 65, 128 and 129 reads: the rounds of 64 lanes at their edges",
                 ref, reads, var)


def _placement():
    ref = make_ref(700, 2)
    reads = [rd(ref, 100, "30M"), rd(ref, 400, "30M", rev=True)]
    var = [snv(ref, p) for p in (5, 99, 100, 129, 130, 300, 400, 429, 430, 650, 699, 0)]
    var += [snv(ref, 129, key=True), snv(ref, 100, key=True)]
    return _case("placement", "a site before the first read, after the last, in a gap; a read's exclusive end (not covered), its "
                 "last base (a tail) and its first base; the contig's two ends", ref, reads, var)


def _del_keys():
    ref = make_ref(700, 3)
    ref = ref[:200] + ref[200:210].lower() + ref[210:]
    reads = [rd(ref, 185, "15M4D10M"), rd(ref, 190, "10M4D10M"), rd(ref, 190, "10M4D10M", rev=True), rd(ref, 190, "10M3D10M"),
             rd(ref, 685, "10M5D"), rd(ref, 685, "10M5D", rev=True), rd(ref, 685, "10M8D"), rd(ref, 686, "9M4D1M")]
    b, e = ref[199], ref[694]
    var = [(199, b + ref[200:204].upper(), b, 0.3, False),      # the key is upper-cased: an upper-case REF matches ...
           (199, b + ref[200:204], b, 0.3, False),              # ... the contig's own lower-case letters do not
           (199, b + ref[200:203].upper(), b, 0.3, False), (199, b + ref[200:205].upper(), b, 0.3, False),
           (694, e + ref[695:700], e, 0.3, False),              # runs to the contig's last base
           (694, e + ref[695:700] + "NNN", e, 0.3, False),      # ... and past it: N beyond ref_len
           (694, e + ref[695:699], e, 0.3, False), (694, e + ref[695:700] + "NN", e, 0.3, False),
           snv(ref, 199), snv(ref, 202), snv(ref, 699), snv(ref, 697)]
    return _case("del_keys", "deletion keys at the contig's edge and across letter case", ref, reads, var)


def _long_window():
    ref = make_ref(700, 4)
    reads = [rd(ref, 0, "400M", qual=35)]
    reads += [rd(ref, 5 + i, "6M", qual=10 + i % 30, rev=i % 2) for i in range(200)]
    reads += [rd(ref, 375, "10M", qual=5 + i % 36, rev=i % 2, sub={380: other(ref[380])} if i % 4 == 0 else None) for i in range(70)]
    var = [snv(ref, 350), snv(ref, 380, af=0.3), snv(ref, 399), snv(ref, 399, key=True), snv(ref, 400), snv(ref, 100), snv(ref, 7)]
    return _case("long_window", "one 400M read first, 200 short reads that end before the site: the window spans rounds whose "
                 "lanes mostly find no overlap, and the ranks carry across rounds", ref, reads, var)


def _wide():
    ref = make_ref(700, 5)
    n = 4300
    reads = [rd(ref, 10 + i * 600 // n, "8M", qual=3 + i % 38, rev=i % 2, mapq=60 if i % 7 else 255,
                sub={300: other(ref[300])} if i % 5 == 0 else None) for i in range(n)]
    var = [snv(ref, reads[0]["pos0"]), snv(ref, 300, af=0.25), snv(ref, reads[-1]["pos0"] + 7), snv(ref, reads[-1]["pos0"]),
           snv(ref, 9), snv(ref, 617)]
    return _case("wide", "4 300 reads (above 65 * 65: the wave-wide search takes two probe rounds), sites at the first, a middle "
                 "and the last read", ref, reads, var)


def _in_ops():
    ref = make_ref(700, 6)
    q2 = lambda n, i: [30] * i + [2] + [30] * (n - i - 1)
    reads = [rd(ref, 100, "10M5D10M"), rd(ref, 100, "10M20N10M", rev=True), rd(ref, 100, "8M3I12M", ins="ACG"),
             rd(ref, 100, "4S20M"), rd(ref, 100, "8M3I12M", ins="ACG", qual=q2(23, 7)),
             rd(ref, 100, "10M5D10M", qual=q2(20, 9), rev=True), rd(ref, 100, "8M2P3I12M", ins="ACG"),
             rd(ref, 100, "10M5D2I10M", ins="TT"), rd(ref, 100, "5=1X14M"), rd(ref, 100, "8M3I12M", ins="ACT"),
             rd(ref, 100, "8M2I13M", ins="AC"), rd(ref, 101, "9M5D3S")]
    b7, b9 = ref[107], ref[109]
    var = [snv(ref, p, af=0.3) for p in (100, 105, 107, 109, 112, 114, 115, 119, 129)]
    var += [(107, b7, b7 + "ACG", 0.3, False), (107, b7, b7 + "ACT", 0.3, False), (107, b7, b7 + "AC", 0.3, False),
            (107, b7, b7 + "ACGT", 0.3, False), (107, b7, other(b7), 0.3, True),
            (109, ref[109:115], b9, 0.3, False), (109, ref[109:114], b9, 0.3, False),
            # an I behind a D: the entry is the deletion's last position, htslib's qpos there is the NEXT base -- the first
            # inserted one -- and the key starts one base later (plp.c:1092 reads qpos + j): "T" + the base behind the insertion
            (114, ref[114], ref[114] + "T" + ref[115], 0.3, False), (114, ref[114], ref[114] + "T" + other(ref[115]), 0.3, False)]
    return _case("in_ops", "a site inside a D and inside an N, behind an I (query shift), behind soft clips, at the last base before "
                 "an I and before a D -- also with BQ 2 there: still an event carrier, not in the column --, a P before the I, "
                 "an I behind a D, = and X", ref, reads, var)


def _ambiguity():
    ref = make_ref(700, 7)
    reads = [rd(ref, 100, "8M3I12M", ins="ARA"), rd(ref, 100, "8M3I12M", ins="ARA", rev=True), rd(ref, 100, "8M3I12M", ins="ANA"),
             rd(ref, 100, "8M3I12M", ins="AAA"), rd(ref, 100, "8M3I12M", ins="A=B"), rd(ref, 100, "20M", sub={107: "R", 110: "N"})]
    b = ref[107]
    var = [(107, b, b + k, 0.2, False) for k in ("ARA", "ANA", "AAA", "A=B", "ara", "AGA")] + [snv(ref, 107), snv(ref, 110)]
    return _case("ambiguity", "ambiguity codes in an insertion are their own letter in the key; in a column they are N", ref, reads, var)


def _quals():
    ref = make_ref(700, 8)
    reads = [rd(ref, 100, "10M", qual=[30] * 5 + [q] + [30] * 4, sub={105: other(ref[105])} if q in (3, 94) else None, rev=q == 93)
             for q in (2, 3, 93, 94, 255)]
    return _case("quals", "BQ 2 (below min_plp_bq), 3 (kept), 93, 94 and 255 (both written as 93)", ref, reads,
                 [snv(ref, 105, af=0.2), snv(ref, 104)])


@functools.lru_cache(None)
def _mixed_reads():
    ref = make_ref(700, 9)
    rng = np.random.default_rng(10)
    reads = []
    for p in sorted(int(x) for x in rng.integers(0, 640, 150)):
        c = ["40M", "20M2I18M", "20M3D20M", "3S37M", "15M10N25M"][int(rng.integers(0, 5))]
        n = sum(l for o, l in parse_cigar(c) if o in "MIS")
        reads.append(rd(ref, p, c, qual=[int(q) for q in rng.integers(2, 42, n)], rev=bool(rng.integers(0, 2)),
                        mapq=int(rng.choice([60, 60, 20, 255]))))
    return ref, reads


def _site_counts():
    ref, reads = _mixed_reads()
    rng = np.random.default_rng(11)
    out = []
    for n in (1, 4, 5, 257):
        pos = [int(p) for p in rng.integers(0, 700, n)]
        var = [snv(ref, p, af=float(rng.choice([0.01, 0.1, 0.5])), k=1 + i % 3, key=(i % 11 == 0)) for i, p in enumerate(pos)]
        out.append(_case("sites_%d" % n, "%d sites in no order, duplicates allowed: the last block of four wavefronts full, "
                         "one over, many blocks" % n, ref, reads, var))
    pos = list(range(650, 50, -17))
    out.append(_case("sites_descending", "sites in descending order", ref, reads, [snv(ref, p) for p in pos]))
    out.append(_case("site_three_alts", "one site three times with three alts", ref, reads,
                     [snv(ref, 333, k=1), snv(ref, 333, k=2), snv(ref, 333, k=3)]))
    return out


def _af_values():
    ref = make_ref(700, 12)
    reads = [rd(ref, 100, "10M4I20M" if i % 5 == 0 else "30M", ins="GGCC", sub={109: other(ref[109])} if i % 4 == 0 else None,
                rev=i % 2) for i in range(20)]
    b = ref[109]
    var = [snv(ref, 109, af=a) for a in (0.0, 1.0, -0.3, 1.7)] + [(109, b, b + "GGCC", a, False) for a in (0.0, 1.0, -0.3, 1.7)]
    return _case("af_values", "AF 0, 1 and the two out-of-range values the reference resets (-0.3 -> 0.01, 1.7 -> 1.0)", ref, reads, var)


def _all_tails():
    ref = make_ref(700, 13)
    reads = [rd(ref, 200 - 10 - 3 * i, "%dM" % (11 + 3 * i), qual=25 + i, rev=i % 2) for i in range(5, -1, -1)]
    more = sorted(reads + [rd(ref, 195, "20M")], key=lambda r: r["pos0"])
    var = [snv(ref, 200), snv(ref, 200, key=True), (200, ref[200:203], ref[200], 0.1, False), snv(ref, 199, key=True)]
    return [_case("all_tails", "every read ends at the site: an SNV keeps its coverage, an indel variant has coverage 0 -- no tag, "
                  "and with --use-det-lim a non-empty column that is not detectable", ref, reads, var),
            _case("all_but_one_tails", "the same with one read that goes on: the indel coverage is 1", ref, more, var)]


@functools.lru_cache(None)
def cases():
    return ([_windows(), _placement(), _del_keys(), _long_window(), _wide(), _in_ops(), _ambiguity(), _quals()] + _site_counts()
            + [_af_values()] + _all_tails())


def case_ids():
    return [c["name"] for c in cases()]


# ---- the oracle road ---------------------------------------------------------------------------------------------------

def is_indel(v):
    return len(v[1]) > 1 or len(v[2]) > 1 or bool(v[4])


def indel_key(v):
    """(side, key) find_ins_sequence / find_del_sequence are asked for (lofreq_uniq.c:343-368): side 1 = deletion"""
    return (1, v[1][1:]) if len(v[1]) > len(v[2]) else (0, v[2][1:])


def ref_base_of(ref, p):
    b = ref[p] if p < len(ref) else "N"
    return ord(b) if b in "ACGTN" else ord("N")          # plp.c:818-823


def oracle_sites(orc, reads, ref, positions, min_plp_bq=3):
    """pileup_region over the whole contig picked at `positions` -> dict(nt, bq, mq, col_off, ref_base, cov, nb, tails,
    events = per site [{key: count}, {key: count}])"""
    P = orc.pack_reads(reads, ref.encode())
    R = orc.pileup_region(P, 0, len(ref), min_plp_bq, 0, use_baq=False)
    H, F = R["host"], R["flat"]
    col_of = {int(p): i for i, p in enumerate(R["col_pos"])}
    nt, bq, mq, off, rb, cov, nb, tails, events = [], [], [], [0], [], [], [], [], []
    for p in positions:
        ci = col_of.get(int(p))
        ev = [{}, {}]
        if ci is None:
            rb.append(ref_base_of(ref, p))
            cov.append(0), nb.append(0), tails.append(0)
        else:
            o0, o1 = int(H["col_off"][ci]), int(H["col_off"][ci + 1])
            nt.append(H["nt"][o0:o1]), bq.append(H["bq"][o0:o1]), mq.append(H["mq"][o0:o1])
            rb.append(int(H["ref_base"][ci]))
            cov.append(int(H["coverage_plp"][ci])), nb.append(int(H["num_bases"][ci])), tails.append(int(F["num_tails"][ci]))
            assert o1 - o0 == nb[-1]
            for s in (0, 1):
                for e in range(int(F["ev_off"][s][ci]), int(F["ev_off"][s][ci + 1])):
                    key = F["key_chars"][s][int(F["key_off"][s][e]):int(F["key_off"][s][e + 1])].decode()
                    ev[s][key] = int(F["rd_off"][s][e + 1] - F["rd_off"][s][e])
        off.append(off[-1] + nb[-1])
        events.append(ev)
    cat = lambda a: np.concatenate(a).astype(np.uint8) if a else np.zeros(0, np.uint8)
    return dict(nt=cat(nt), bq=cat(bq), mq=cat(mq), col_off=np.asarray(off, np.uint64), ref_base=np.asarray(rb, np.uint8),
                cov=np.asarray(cov, np.int32), nb=np.asarray(nb, np.int32), tails=np.asarray(tails, np.int32), events=events)


def oracle_uniq(orc, S, variants, af=None):
    """uniq_snv on the picked columns S for `variants` [(pos0, REF, ALT, af, INDEL key)] -> dict(coverage, alt_count, uq,
    pvalue, detectable, detlim_pvalue); af: one value for all (--uni-freq) or None"""
    n = len(variants)
    afs = np.asarray([(v[3] if af is None else af) for v in variants], np.float32)
    ind = np.asarray([is_indel(v) for v in variants], bool)
    coverage = (S["cov"] - np.where(ind, S["tails"], 0)).astype(np.int32)                     # lofreq_uniq.c:248-251
    alt_count = np.zeros(n, np.int32)
    uq = np.full(n, -1, np.int32)
    pv = np.full(n, -1.0)
    pad = lambda a: np.concatenate([a, np.zeros(32, np.uint8)])
    if n:
        s_uq, s_pv = orc.uniq_binom_batch(pad(S["nt"]), S["col_off"], afs, "".join((v[2][:1] or "N") for v in variants),
                                          coverage_plp=S["cov"])
        cnt = [0 if not ind[i] else S["events"][i][indel_key(variants[i])[0]].get(indel_key(variants[i])[1], 0) if
               indel_key(variants[i])[1] else 0 for i in range(n)]
        f_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        i_uq, i_pv = orc.uniq_binom_batch(np.zeros(int(f_off[-1]) + 32, np.uint8), f_off, afs, "A" * n, coverage_plp=coverage)
        for i in range(n):
            if coverage[i] < 1:
                continue
            if ind[i]:
                alt_count[i], uq[i], pv[i] = cnt[i], i_uq[i], i_pv[i]
            else:
                code = "ACGT".find(variants[i][2][:1].upper())
                col = S["nt"][int(S["col_off"][i]):int(S["col_off"][i + 1])] & 7
                alt_count[i] = int((col == code).sum()) if code >= 0 else int((col > 3).sum())
                uq[i], pv[i] = s_uq[i], s_pv[i]
    flag, dpv = (orc.uniq_detlim_batch(pad(S["nt"]), pad(S["bq"]), None, pad(S["mq"]), None, S["col_off"], S["ref_base"], afs)
                 if n else (np.zeros(0, np.uint8), np.zeros(0, np.longdouble)))
    det = (flag.astype(bool) & (coverage >= 1)).astype(np.uint8)                              # :252-254 comes first
    return dict(coverage=coverage, alt_count=alt_count, uq=uq, pvalue=pv, detectable=det, detlim_flag=flag, detlim_pvalue=dpv)


# ---- tests/golden/uniq_reads.json (tests/make_uniq_reads_golden.py) -------------------------------------------------------

def load_uniq_reads():
    """-> (fixture, contig, the reads uniq's mpileup keeps -- uniq_filter applied HERE, as a caller of the read set has to --,
    variants [(pos0, REF, ALT, float32 AF, INDEL key)])"""
    fx = json.load(open(os.path.join(HERE, "golden", "uniq_reads.json")))
    reads = []
    for pos0, flag, mapq, cigar, seq, qual in fx["reads"]:
        if uniq_filter(flag, mapq):
            reads.append({"pos0": pos0, "cigar": parse_cigar(cigar), "seq": np.asarray([CODE.get(c, 4) for c in seq], np.uint8),
                          "qual": np.asarray([ord(c) - 33 for c in qual], np.uint8), "mapq": mapq, "reverse": bool(flag & 16)})
    var = [(v["pos0"], v["ref"], v["alt"], np.float32(v["af"]), v["indel_key"]) for v in fx["variants"]]
    return fx, fx["genome"], reads, var


def binary_run(fx, run):
    """-> (uq with -1 for no tag, UNIQ flags, PASS flags) the 2.1.4 binary wrote in `run`"""
    r = [v["runs"][run] for v in fx["variants"]]
    return ([(-1 if x["uq"] is None else x["uq"]) for x in r], [bool(x["uniq"]) for x in r], [x["filter"] == "PASS" for x in r])
