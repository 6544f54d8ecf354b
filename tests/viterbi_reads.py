"""Seeded reads for the viterbi realigner (tests/golden/viterbi_*.json, tests/test_viterbi_model.py, tests/test_gpu_viterbi.py).

One contig with AT / CAG repeats, homopolymers, a few N and a lower-case stretch; reads of 36 to 340 bases in the shapes
`lofreq viterbi` has to deal with:
  repeat   one insertion or deletion of repeat units inside a repeat, written at its RIGHTMOST place (the realigner moves it left)
  random   one indel anywhere, deletions up to 30 bases
  shifted  the read is reported 1-4 bases off its start, with a compensating leading I or an early D
  edge     an I as the first or the last operation
  double   two indels
  plain    no indel; and an H-clipped, an N-operation and an all-Q2 read with an indel (all four are left untouched)
on top of which come soft clips, = / X instead of M, runs of Q2 bases, a quality of 0, N and IUPAC read bases, and reads whose
window is clipped at either end of the contig."""
import hashlib

import numpy as np

GENERATOR_VERSION = 1
LETTERS = "ACGTN=MRSVWYHKDB"
_CODE = {c: i for i, c in enumerate(LETTERS)}
LENGTHS = (36, 75, 150, 250, 340)


def make_genome(rng, glen):
    g = list(rng.choice(list("ACGT"), glen))
    x = 25
    kind = 0
    while x + 40 < glen - 25:
        n = int(rng.integers(4, 13))
        unit = ("AT", "A", "CAG", "T", "TA", "G")[kind % 6]
        rep = (unit * n)
        g[x:x + len(rep)] = rep
        x += len(rep) + int(rng.integers(18, 45))
        kind += 1
    for p in rng.integers(30, glen - 30, max(glen // 600, 1)):
        g[int(p)] = "N"
    lo = glen // 3
    g[lo:lo + 120] = [c.lower() for c in g[lo:lo + 120]]
    return "".join(g)


def _repeats(genome):
    """[(start, end, unit length)] of the planted repeats, found again by scanning"""
    G = genome.upper()
    out = []
    i = 0
    while i < len(G) - 8:
        for u in (1, 2, 3):
            j = i + u
            while j < len(G) and G[j] == G[j - u]:
                j += 1
            if j - i >= max(4 * u, 6) and G[i] != "N":
                out.append((i, j, u))
                i = j - 1
                break
        i += 1
    return out


def _walk(rng, genome, p, ops):
    """ops [(op, len, inserted bases or None)] -> read letters; M copies the contig"""
    seq, x = [], p
    for op, ln, ins in ops:
        if op == "M":
            seq.extend(genome[x:x + ln].upper())
            x += ln
        elif op == "Mfix":                      # bases given, aligned to the contig whatever it holds
            seq.extend(ins)
            x += ln
        elif op in "IS":
            seq.extend(ins if ins is not None else rng.choice(list("ACGT"), ln))
        elif op in "DN":
            x += ln
    return seq, x


def _rightmost(genome, p, ops, seq):
    """[M a][I | D l][M b]: move the indel right while the alignment stays as good"""
    (_, a, _), (op, l, ins), (_, b, _) = ops
    G = genome.upper()
    if op == "D":
        d = p + a
        while b > 2 and d + l < len(G) and G[d] == G[d + l]:
            a, b, d = a + 1, b - 1, d + 1
    else:
        while b > 2 and seq[a] == seq[a + l]:
            a, b = a + 1, b - 1
    return [("M", a, None), (op, l, ins), ("M", b, None)]


def _eqx(genome, p, ops, seq):
    out, x, y = [], p, 0
    G = genome.upper()
    for op, ln, ins in ops:
        if op == "M":
            for j in range(ln):
                o = "=" if seq[y + j] == G[x + j] else "X"
                if out and out[-1][0] == o:
                    out[-1] = (o, out[-1][1] + 1)
                else:
                    out.append((o, 1))
            x += ln
            y += ln
        else:
            out.append((op, ln))
            if op in "IS":
                y += ln
            elif op in "DN":
                x += ln
    return out


def make(seed, n, glen=2400):
    """-> {"genome": str, "reads": [{name, pos0, cigar [(op, len)], seq (letters), qual [phred], shape}]}"""
    rng = np.random.default_rng(seed)
    genome = make_genome(rng, glen)
    reps = _repeats(genome)
    reads = []
    shapes = ["repeat"] * 8 + ["random"] * 3 + ["shifted"] * 4 + ["edge"] * 1 + ["double"] * 1 + ["plain", "hclip", "nop", "allq2"]
    for r in range(n):
        L = int(LENGTHS[int(rng.choice(5, p=[0.3, 0.3, 0.25, 0.1, 0.05]))])
        shape = shapes[int(rng.integers(len(shapes)))] if r >= 40 else ["plain", "hclip", "nop", "allq2", "repeat"][r % 5]
        lead = int(rng.integers(1, 9)) if rng.random() < 0.2 else 0
        trail = int(rng.integers(1, 9)) if rng.random() < 0.2 else 0
        body = L - lead - trail
        pos_hint = rng.random()
        span_max = body + 40
        if pos_hint < 0.04:
            p = int(rng.integers(0, 9))
        elif pos_hint < 0.08:
            p = glen - span_max + int(rng.integers(30, 40))
        else:
            p = int(rng.integers(10, glen - span_max - 10))
        ops = None
        if shape in ("repeat", "hclip", "allq2"):
            cand = [(s, e, u) for s, e, u in reps if s >= p + 6 and e <= p + body - 6]
            if cand:
                s, e, u = cand[int(rng.integers(len(cand)))]
                units = int(rng.integers(1, 3))
                l = u * units
                at = int(rng.integers(s, e - l + 1)) if e - l > s else s
                a = at - p
                if rng.random() < 0.5 and e - s >= l + u:
                    ops = [("M", a, None), ("D", l, None), ("M", body - a, None)]
                else:
                    ops = [("M", a, None), ("I", l, list(genome[s:s + l].upper())), ("M", body - a - l, None)]
            else:
                shape = "random" if shape == "repeat" else shape
        if ops is None and shape in ("random", "hclip", "allq2", "nop"):
            a = int(rng.integers(3, body - 8))
            if rng.random() < 0.5:
                ops = [("M", a, None), ("D", int(rng.integers(1, 31)), None), ("M", body - a, None)]
            else:
                l = int(rng.integers(1, min(9, body - a - 2)))
                ops = [("M", a, None), ("I", l, None), ("M", body - a - l, None)]
        if shape == "nop":
            a = ops[0][1]
            cut = max(a // 2, 1)
            ops = [("M", cut, None), ("N", int(rng.integers(20, 200)), None), ("M", a - cut, None)] + ops[1:] if a - cut > 0 else ops
            if ops[1][0] != "N":
                ops = [("M", 1, None), ("N", 30, None)] + [("M", ops[0][1] - 1, None)] + ops[1:]
        if shape == "shifted":
            d = int(rng.integers(1, 5))
            if rng.random() < 0.5 or p < d + 1:
                # the read really starts at p with `body` matches; reported d to the right with its first d bases inserted
                true_seq, _ = _walk(rng, genome, p, [("M", body, None)])
                ops = [("I", d, true_seq[:d]), ("M", body - d, None)]
                p_rep = p + d
            else:
                # reported d to the left: one base (aligned where the contig holds something else), a deletion of d, the rest
                true_seq, _ = _walk(rng, genome, p, [("M", body, None)])
                ops = [("Mfix", 1, true_seq[:1]), ("D", d, None), ("M", body - 1, None)]
                p_rep = p - d
            p = p_rep
        if shape == "edge":
            l = int(rng.integers(1, 5))
            ops = [("I", l, None), ("M", body - l, None)] if rng.random() < 0.5 else [("M", body - l, None), ("I", l, None)]
        if shape == "double":
            a = int(rng.integers(4, body // 3))
            b = int(rng.integers(4, body // 3))
            l1, l2 = int(rng.integers(1, 4)), int(rng.integers(1, 4))
            ops = [("M", a, None), ("I", l1, None), ("M", b, None), ("D", l2, None), ("M", body - a - l1 - b, None)]
        if shape == "plain":
            ops = [("M", body, None)]
        seq, x_end = _walk(rng, genome, p, ops)
        ops = [("M" if o == "Mfix" else o, l, i) for o, l, i in ops]
        if x_end > glen or p < 0:
            ops = [("M", body, None)]
            p = min(max(p, 0), glen - body)
            seq, x_end = _walk(rng, genome, p, ops)
            shape = "plain"
        if shape in ("repeat", "random") and len(ops) == 3:
            ops = _rightmost(genome, p, ops, seq)
        # sequencing errors, ambiguity codes
        for j in range(len(seq)):
            u = rng.random()
            if u < 0.01:
                seq[j] = "ACGT"[int(rng.integers(4))]
            elif u < 0.012:
                seq[j] = "N"
            elif u < 0.013:
                seq[j] = "MRSVWYHKDB"[int(rng.integers(10))]
        qual = [int(v) for v in rng.integers(8, 42, len(seq))]
        if rng.random() < 0.15:
            t = int(rng.integers(2, max(len(seq) // 3, 3)))
            qual[-t:] = [2] * t
        if rng.random() < 0.05:
            j = int(rng.integers(len(seq)))
            qual[j:j + 3] = [2] * len(qual[j:j + 3])
        if rng.random() < 0.04:
            qual[int(rng.integers(len(seq)))] = 0
        if rng.random() < 0.02:
            qual[int(rng.integers(len(seq)))] = 93
        if shape == "allq2":
            qual = [2] * len(seq)
        cig = _eqx(genome, p, ops, seq) if rng.random() < 0.1 and shape != "shifted" else [(o, l) for o, l, _ in ops]
        merged = []
        for o, l in cig:
            if l <= 0:
                continue
            if merged and merged[-1][0] == o:
                merged[-1] = (o, merged[-1][1] + l)
            else:
                merged.append((o, l))
        cig = merged
        if lead:
            cig = [("S", lead)] + cig
            seq = list(rng.choice(list("ACGT"), lead)) + seq
            qual = [int(v) for v in rng.integers(2, 30, lead)] + qual
        if trail:
            cig = cig + [("S", trail)]
            seq = seq + list(rng.choice(list("ACGT"), trail))
            qual = qual + [int(v) for v in rng.integers(2, 30, trail)]
        if shape == "hclip":
            cig = [("H", 5)] + cig
        reads.append({"name": "r%d" % r, "pos0": int(p), "cigar": cig, "seq": "".join(seq), "qual": qual, "shape": shape})
    return {"genome": genome, "reads": reads}


def sam_text(genome, reads):
    out = ["@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:chr1\tLN:%d\n" % len(genome)]
    for r in reads:
        out.append("%s\t0\tchr1\t%d\t60\t%s\t*\t0\t0\t%s\t%s\n" % (
            r["name"], r["pos0"] + 1, "".join("%d%s" % (l, o) for o, l in r["cigar"]), r["seq"],
            "".join(chr(33 + q) for q in r["qual"])))
    return "".join(out)


def sha256(text):
    return hashlib.sha256(text.encode()).hexdigest()


def lib_read(r):
    """the dict lofreq_amd.baq.baq_batch / viterbi_batch and tests/viterbi_model.py take"""
    return {"pos0": r["pos0"], "cigar": [tuple(c) for c in r["cigar"]],
            "seq": np.asarray([_CODE[c] for c in r["seq"]], np.uint8), "qual": np.asarray(r["qual"], np.uint8)}


def has_q2(r):
    """whether -q can matter to the read at all: a base of quality 2 in its query"""
    return 2 in r["qual"]
