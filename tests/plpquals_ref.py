"""Plain-Python restatement of the quality lines of `lofreq plpsummary` (plp_summary, lofreq_call.c:460-598) from reads, on top of
the cursor walk of tests/plpsummary_ref.py: what compile_plp_col (plp.c:841-1194) files per column under base_quals[nt4] /
baq_quals[nt4] / map_quals[nt4] / source_quals[nt4], ins_quals / ins_map_quals, del_quals / del_map_quals and the ins / del event
tables, and how plp_summary prints them.  Also the same grouping stated on SNV TRACKS (group_tracks), which is what
lfq_plp_group_kernel computes.  Test infrastructure, no device.

Reads are the dicts of lofreq_amd.ReadSet (see plpsummary_ref.py) with the optional tag bytes lb, ai, ad (quality + 33) and "sq",
the read's source quality as the reference keeps it in its sq tag (an int; 49314 for an error probability of 0.0)."""
import plpsummary_ref as ref

NT4 = ref.NT4
LFQ_USE_BAQ, LFQ_USE_SQ = 1, 4
SQ_ZERO_PROB = 49314            # PROB_TO_PHREDQUAL(LDBL_MIN): what source_qual returns for a read without a counted mismatch


def columns(reads, genome, begin, end, min_plp_bq=3, min_plp_idq=0, keep=None, use_baq=True, use_sq=False):
    """-> {pos0: column}: nt = five lists of (bq, baq, mq, sq) in pileup order; ne = per side [(idq, mq)] of the reads without an
    event of that side; ev = per side {key: [(q, mq, aq, sq)]} in order of first appearance"""
    reads = [r for i, r in enumerate(reads) if keep is None or keep[i]]
    cursors = [ref.Cursor(r) for r in reads]
    cols = {}
    first = 0
    for p in range(begin, end):
        nt = [[] for _ in range(5)]
        ne = [[], []]
        ev = [{}, {}]
        cov = 0
        while first < len(reads) and cursors[first].end <= p:
            first += 1
        for r, c in zip(reads[first:], cursors[first:]):
            if r["pos0"] > p:
                break
            e = c.entry(p)
            if e is None:
                continue
            is_del, qpos, indel, _, _ = e
            cov += 1
            mq = int(r["mapq"])                                       # plp.c:909
            sq = int(r["sq"]) if use_sq else -1                       # :861, 882-884
            if not is_del:
                code = int(r["seq"][qpos])
                nt4 = code if code < 4 else 4
                bq = int(r["qual"][qpos])
                if bq >= min_plp_bq:                                  # :937
                    bq = min(bq, ref.SANGER_PHRED_MAX)                # :949-953
                    baq = None
                    if use_baq:                                       # :956-962
                        baq = int(r["lb"][qpos]) - 33 if r.get("lb") is not None else -1
                    nt[nt4].append((bq, baq, mq, sq))
            iq = int(r["bi"][qpos]) - 33 if r.get("bi") is not None else 0       # :1024-1059
            dq = int(r["bd"][qpos]) - 33 if r.get("bd") is not None else 0
            if iq < min_plp_idq or dq < min_plp_idq:                  # :1062
                continue
            if indel > 0:                                             # :1072-1112
                aq = int(r["ai"][qpos]) - 33 if r.get("ai") is not None else -1
                key = "".join(ref.SEQ_LETTERS[int(r["seq"][qpos + j])] if qpos + j < len(r["seq"]) else "N"
                              for j in range(1, indel + 1))
                ev[0].setdefault(key, []).append((iq, mq, aq, sq))
                ne[1].append((dq, mq))
            elif indel < 0:                                           # :1116-1168
                aq = int(r["ad"][qpos]) - 33 if r.get("ad") is not None else -1
                key = "".join(genome[p + j].upper() if p + j < len(genome) else "N" for j in range(1, -indel + 1))
                ev[1].setdefault(key, []).append((dq, mq, aq, sq))
                ne[0].append((iq, mq))
            else:                                                     # :1170-1191
                ne[0].append((iq, mq))
                ne[1].append((dq, mq))
        if cov:
            cols[p] = {"nt": nt, "ne": ne, "ev": ev}
    return cols


def _line(head, title, vals):
    return "  %s\t%s =\t%s\n" % (head, title, "".join(" %d" % v for v in vals))


def format_nt(nt, use_baq=True, use_sq=False):
    """lofreq_call.c:460-489; nt = five lists of (bq, baq, mq, sq)"""
    s = ""
    for i in range(5):
        if not nt[i]:                                                 # :466
            continue
        s += _line(NT4[i], "BQ", [v[0] for v in nt[i]])
        s += _line(NT4[i], "BAQ", [v[1] if use_baq else -1 for v in nt[i]])      # :475-479
        s += _line(NT4[i], "MQ", [v[2] for v in nt[i]])
        if use_sq:
            s += _line(NT4[i], "SQ", [v[3] for v in nt[i]])
    return s


def format_indels(ne, ev):
    """lofreq_call.c:491-598, the closing empty line included"""
    s = ""
    for sd, t in enumerate("+-"):
        s += _line(t + "0", "IDQ", [v[0] for v in ne[sd]])
        s += _line(t + "0", "MQ", [v[1] for v in ne[sd]])
        for key, rd in ev[sd].items():
            s += _line(t + key, "IQ" if sd == 0 else "IDQ", [v[0] for v in rd])
            s += _line(t + key, "MQ", [v[1] for v in rd])
            s += _line(t + key, "AQ", [v[2] for v in rd])
            s += _line(t + key, "SQ", [v[3] for v in rd])
    return s + "\n"


def text(chrom, reads, genome, begin, end, flag=LFQ_USE_BAQ, min_plp_bq=3, min_plp_idq=0, keep=None):
    """the stdout of `lofreq plpsummary` for the region -> list of one string per covered position"""
    use_baq, use_sq = bool(flag & LFQ_USE_BAQ), bool(flag & LFQ_USE_SQ)
    heads = ref.summarize(reads, genome, begin, end, min_plp_bq, min_plp_idq, keep)
    cols = columns(reads, genome, begin, end, min_plp_bq, min_plp_idq, keep, use_baq, use_sq)
    assert [h["pos0"] for h in heads] == sorted(cols)
    return [ref.format_line(chrom, h) + format_nt(cols[h["pos0"]]["nt"], use_baq, use_sq)
            + format_indels(cols[h["pos0"]]["ne"], cols[h["pos0"]]["ev"]) for h in heads]


# ---- the same on SNV tracks (include/lofreq_amd.h: nt bits 0-2 code, bit 3 strand; 255 = missing for baq / sq, 254 = 49314 for sq)

def group_tracks(nt, bq, baq, mq, sq, col_off, c0, c1):
    """the stable partition lfq_plp_group_kernel computes for the columns [c0, c1): -> (nt_off [5 * n + 1], bq, baq, mq, sq), the
    grouped bytes as lists (baq / sq None where the tracks have none)"""
    base = int(col_off[c0])
    nt_off, order = [], []
    for c in range(c0, c1):
        obs = range(int(col_off[c]), int(col_off[c + 1]))
        for k in range(5):
            nt_off.append(len(order))
            order.extend(i for i in obs if min(int(nt[i]) & 7, 4) == k)
    nt_off.append(len(order))
    assert len(order) == int(col_off[c1]) - base
    pick = lambda a: None if a is None else [int(a[i]) for i in order]
    return nt_off, pick(bq), pick(baq), pick(mq), pick(sq)


def format_grouped(nt_off, bq, baq, mq, sq, i, flag):
    """lofreq_call.c:460-489 for column i of a group_tracks result, with the decoding of the track bytes"""
    use_baq, use_sq = bool(flag & LFQ_USE_BAQ), bool(flag & LFQ_USE_SQ)
    groups = []
    for k in range(5):
        a, b = nt_off[5 * i + k], nt_off[5 * i + k + 1]
        groups.append([(bq[j], (-1 if baq[j] == 255 else baq[j]) if use_baq else -1, mq[j],
                        (-1 if sq[j] == 255 else SQ_ZERO_PROB if sq[j] == 254 else sq[j]) if use_sq else -1) for j in range(a, b)])
    return format_nt(groups, use_baq, use_sq)


def load_golden(name):
    """tests/golden/<name>.json (tests/make_plpquals_golden.py) -> (fixture, reads as dicts with bi / bd / lb / ai / ad, the text cut
    into one string per column)"""
    import json
    import os

    import numpy as np
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".json")))
    code = {c: i for i, c in enumerate(ref.SEQ_LETTERS)}
    tag = lambda t: None if t is None else np.frombuffer(t.encode(), np.uint8)
    reads = [{"pos0": r[0], "cigar": ref._parse_cigar(r[3]), "seq": np.array([code.get(c, 4) for c in r[4].upper()], np.uint8),
              "qual": np.array([ord(c) - 33 for c in r[5]], np.uint8), "mapq": r[2], "reverse": bool(r[1] & 16),
              "bi": tag(r[6]), "bd": tag(r[7]), "lb": tag(r[8]), "ai": tag(r[9]), "ad": tag(r[10])} for r in fx["reads"]]
    blocks = [b + "\n\n" for b in fx["text"].split("\n\n") if b]
    assert "".join(blocks) == fx["text"]
    return fx, reads, blocks


def flag_of(fx):
    return LFQ_USE_BAQ | (LFQ_USE_SQ if "-s" in fx["args"] else 0)


def source_quals(oracle, reads, genome):
    """the reads' sq tags as mplp_func stores them with -s (plp.c:1349-1360): max(source_qual(), 0) with the defaults of
    `lofreq plpsummary` (no -T: def_nm_q -1; min_bq 6), by the oracle's restatement of source_qual"""
    g = genome.encode()
    return [max(oracle.source_qual(r["pos0"], r["cigar"], np_min4(r["seq"]), r["qual"], g), 0) for r in reads]


def np_min4(seq):
    import numpy as np
    return np.minimum(np.asarray(seq, np.uint8), 4)
