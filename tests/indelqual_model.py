"""Plain-Python model of `lofreq indelqual` (lofreq_indelqual.c:42-215), written from the reference's source: what
tests/test_indelqual_model.py holds against the reference's 2.1.4 binary and tests/test_gpu_indelqual.py against the library.

Dindel mode (dindel_fetch_func, :136-215): the contig is upper-cased (:155); find_homopolymers (:109-133) gives every position a
count -- the run length at the first base of a run of equal letters, 1 at every other position; the CIGAR walk (:173-198) gives
a base aligned to reference position x by M / = / X the letter DINDELQ[count[x + 1]], '!' when x > rlen - 2 or the count is
above 18; D advances x; the bases of I and S get '!'; H does nothing; any other operation is fatal.  BI and BD get the same
string.  Uniform mode (:69-104, 218-258): l_qseq copies of ENCODE_Q(quality + 33) (:66), whatever the read looks like."""

DINDELQ = "!MMMLKEC@=<;:988776"         # lofreq_indelqual.c:42, indexed by the count; 1-based, 18 entries


def homopolymer_counts(ref):
    """find_homopolymers on the upper-cased contig"""
    G = ref.upper()
    count = [1] * len(G)
    i = 0
    while i < len(G):
        j = i + 1
        while j < len(G) and G[j] == G[i]:
            j += 1
        count[i] = j - i
        i = j
    return count


def dindel_table(ref):
    """the letter of every reference position x (what a base aligned to x gets)"""
    count = homopolymer_counts(ref)
    rlen = len(ref)
    return "".join("!" if x > rlen - 2 or count[x + 1] > 18 else DINDELQ[count[x + 1]] for x in range(rlen))


def dindel_read(table, pos0, cigar):
    """cigar: [(op letter, length)] -> the BI (= BD) string; ValueError for an operation the reference dies on"""
    out, x = [], pos0
    for op, l in cigar:
        if op in "M=X":
            out.append("".join(table[p] if p < len(table) else "!" for p in range(x, x + l)))
            x += l
        elif op == "D":
            x += l
        elif op in "IS":
            out.append("!" * l)
        elif op != "H":
            raise ValueError("unknown op %s" % op)
    return "".join(out)


def encode_q(q):
    return "!" if q < 33 else ("~" if q > 126 else chr(q))


def uniform_read(l_qseq, ins_qual, del_qual=None):
    """-u INT[,INT] -> (BI, BD)"""
    del_qual = ins_qual if del_qual is None else del_qual
    return encode_q(ins_qual + 33) * l_qseq, encode_q(del_qual + 33) * l_qseq


def rle(s):
    """"MMMM!L" -> "M4,!1,L1," (the symbol, its count, a comma: a symbol may itself be a digit or a comma)"""
    out, i = [], 0
    while i < len(s):
        j = i
        while j < len(s) and s[j] == s[i]:
            j += 1
        out.append("%s%d," % (s[i], j - i))
        i = j
    return "".join(out)


def unrle(t):
    out, i = [], 0
    while i < len(t):
        j = t.index(",", i + 1)
        out.append(t[i] * int(t[i + 1:j]))
        i = j + 1
    return "".join(out)
