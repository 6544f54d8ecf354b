"""`lofreq viterbi` restated in plain Python doubles: fetch_func (lofreq_viterbi.c:107-345), viterbi and left_align_indels
(viterbi.c:99-330, 48-96), int_median and argmax_d (utils.c:436-457, 87-98).  The CPU checker of lfq_viterbi_batch: the same
log10 / pow calls of the host's libm, the same order of additions, first-maximum ties.  tests/golden/viterbi_*.json hold what
the reference's 2.1.4 binary gives for the same reads (tests/make_viterbi_golden.py).

A read is the dict of lofreq_amd.baq.baq_batch: {pos0, cigar [(op, len)], seq (base codes), qual (phred)}."""
import json
import math
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LETTERS = "ACGTN=MRSVWYHKDB"                # LFQ_SEQ_LETTERS
INT_MIN = float(-2147483648)
RWIN = 10
NO_INDEL, SKIPPED_OP, ALL_Q2, REALIGNED, CHANGED = 0, 1, 2, 3, 8


def int_median(data):
    """utils.c:436-457"""
    if not data:
        return 0
    s = sorted(data)
    n = len(s)
    return int((s[n // 2] + s[n // 2 - 1]) / 2.0) if n % 2 == 0 else s[n // 2]


def _log10(x):
    return math.log10(x) if x > 0.0 else -math.inf         # log10(0) of C


def left_align_indels(ref, query):
    """viterbi.c:48-96 on two lists of characters, in place.  After a shift at index 0 the reference steps back to -1 and
    looks in front of its arrays; here that step changes nothing."""
    slen = len(ref)
    i = 0
    while i < slen - 1:
        if i >= 0 and ref[i] != "*" and query[i] != "*":
            if ref[i + 1] == "*":
                ilen = 0
                while i + 1 + ilen < slen and ref[i + 1 + ilen] == "*":
                    ilen += 1
                if query[i + ilen] == ref[i]:
                    ref[i + ilen] = ref[i]
                    ref[i] = "*"
                    i -= 1
                    continue
            elif query[i + 1] == "*":
                dlen = 0
                while i + 1 + dlen < slen and query[i + 1 + dlen] == "*":
                    dlen += 1
                if query[i] == ref[i + dlen]:
                    query[i + dlen] = query[i]
                    query[i] = "*"
                    i -= 1
                    continue
        i += 1
    return "".join("I" if r == "*" else "D" if q == "*" else "M" for r, q in zip(ref, query))


def viterbi(ref, query, quals, quality):
    """viterbi.c:99-330: (k, state string after left_align_indels)"""
    qlen, rlen = len(query) + 1, len(ref) + 1
    alpha, beta = 0.00001, 0.4
    L = float(rlen)
    gamma = 1 / (2. * L)
    ep_ins = math.log10(.25)
    t_mm = math.log10((1 - 2 * alpha) * (1 - gamma))
    t_mi = math.log10(alpha * (1 - gamma))
    t_md = math.log10(alpha * (1 - gamma))
    t_im = math.log10((1 - beta) * (1 - gamma))
    t_ii = math.log10(beta * (1 - gamma))
    t_dm = math.log10(1 - beta)
    t_dd = math.log10(beta)
    t_sm = math.log10((1 - alpha) / L)
    t_si = math.log10(alpha / L)
    Mp, Ip, Dp = [INT_MIN] * rlen, [INT_MIN] * rlen, [INT_MIN] * rlen       # row i - 1
    ptr = [None]
    for i in range(1, qlen):
        q = quals[i - 1]
        bp = math.pow(10.0, -0.1 * (quality if q == 2 else q))
        ep_match = _log10(1 - bp)
        ep_match_not = _log10(bp / 3.)
        v_start = 0.0 if i == 1 else INT_MIN
        s_m, s_i = v_start + t_sm, v_start + t_si
        qc = query[i - 1]
        M, I, D = [INT_MIN] * rlen, [INT_MIN] * rlen, [INT_MIN] * rlen
        row = bytearray(rlen)
        m_left = d_left = INT_MIN
        for k in range(1, rlen):
            best, pm = s_m, 0
            x = Mp[k - 1] + t_mm
            if x > best:
                best, pm = x, 1
            x = Ip[k - 1] + t_im
            if x > best:
                best, pm = x, 2
            x = Dp[k - 1] + t_dm
            if x > best:
                best, pm = x, 3
            m = (ep_match if qc == ref[k - 1] else ep_match_not) + best
            best, pi = s_i, 0
            x = Mp[k] + t_mi
            if x > best:
                best, pi = x, 1
            x = Ip[k] + t_ii
            if x > best:
                best, pi = x, 2
            I[k] = ep_ins + best
            best, pd = m_left + t_md, 0
            x = d_left + t_dd
            if x > best:
                best, pd = x, 1
            M[k] = m_left = m
            D[k] = d_left = best
            row[k] = pm | pi << 2 | pd << 4
        ptr.append(row)
        Mp, Ip, Dp = M, I, D
    end_state, best_score, best_index = "!", INT_MIN, 0
    for k in range(rlen):
        if Mp[k] > best_score:
            end_state, best_score, best_index = "M", Mp[k], k
        if Ip[k] > best_score:
            end_state, best_score, best_index = "I", Ip[k], k
    i, k, cur = qlen - 1, best_index, end_state
    st, ar, aq = [], [], []
    while i != 0 and k != 0:
        if cur == "S":
            break
        b = ptr[i][k]
        st.append(cur)
        if cur == "M":
            ar.append(ref[k - 1])
            aq.append(query[i - 1])
            cur = "SMID"[b & 3]
            i -= 1
            k -= 1
        elif cur == "I":
            ar.append("*")
            aq.append(query[i - 1])
            cur = "SMI"[(b >> 2) & 3]
            i -= 1
        elif cur == "D":
            ar.append(ref[k - 1])
            aq.append("*")
            cur = "MD"[(b >> 4) & 1]
            k -= 1
        else:
            raise ValueError("no end state")
    ar.reverse()
    aq.reverse()
    return k, left_align_indels(ar, aq)


def realign(read, ref, def_qual=-1):
    """fetch_func for one mapped read -> (pos0, cigar [(op, len)], status); ref: the contig, str or bytes"""
    if isinstance(ref, (bytes, bytearray)):
        ref = ref.decode()
    pos, cigar = int(read["pos0"]), [(o, int(l)) for o, l in read["cigar"]]
    x, y, indels = pos, 0, 0
    query, quals = [], []
    for op, ln in cigar:
        if op in "M=X" or op == "I":
            query.extend(LETTERS[int(c)] for c in read["seq"][y:y + ln])
            quals.extend(int(v) for v in read["qual"][y:y + ln])
            y += ln
            if op == "I":
                indels += 1
            else:
                x += ln
        elif op == "D":
            x += ln
            indels += 1
        elif op == "S":
            y += ln
        else:                                   # H, and N / P: "Not touching read"
            return pos, cigar, SKIPPED_OP
    if indels == 0:
        return pos, cigar, NO_INDEL
    remaining = [v for v in quals if v != 2]
    if not remaining:
        return pos, cigar, ALL_Q2
    q2def = def_qual if def_qual >= 0 else int_median(remaining)
    lower = max(pos - RWIN, 0)
    upper = min(x + RWIN, len(ref))
    k, aln = viterbi(ref[lower:upper].upper(), query, quals, q2def)
    new = []
    if cigar[0][0] == "S":
        new.append(cigar[0])
    if aln:
        new.extend((m.group(0)[0], len(m.group(0))) for m in re.finditer(r"M+|I+|D+", aln))
    else:
        new.append(("D", 1))                    # the empty string's terminator is read as a D (lofreq_viterbi.c:279-295)
    if cigar[-1][0] == "S":
        new.append(cigar[-1])
    new_pos = lower + k
    status = REALIGNED | (CHANGED if (new_pos, new) != (pos, cigar) else 0)
    return new_pos, new, status


def realign_job(job):
    """for a process pool: (read, ref window offset-free contig, def_qual)"""
    read, ref, def_qual = job
    return realign(read, ref, def_qual)


def cigar_str(cigar):
    return "".join("%d%s" % (l, o) for o, l in cigar) or "*"


def parse_cigar(s):
    return [(o, int(l)) for l, o in re.findall(r"(\d+)([MIDNSHP=X])", s)]


def load(name):
    return json.load(open(os.path.join(HERE, "golden", name + ".json")))
