"""A plain Python model of how the 2.1.4 binary reads and writes VCF text and of `lofreq vcfset`, written from the reference's
vcf.c, lofreq_vcfset.c and plp.c (cited per rule), plus the refusals lofreq_amd/csrc/lfq_vcf.h adds.  tests/test_vcf_model.py holds it
to the binary (tests/golden/vcf_binary.json); the header's check program and the device are held to it.

    parse(data, mode)                    -> Parsed, or raises Refused(why, line)
    vcfset(ones, two, **conf)            -> {"counts": (n_vars1, n_ignored, n_out), "keep": [...], "text": bytes}, or raises Refused
    filter_vars(p), uniq_variants(p, ...), ign_mask(p, chrom, ref_len, bed)
"""
import struct

OK, LINE_TOO_LONG, NUL, NUMBER, FIELDS, UNSORTED, INTERVAL, MULTIALLELIC = range(8)
STREAM, TABIX = 0, 1
F_PASSES, F_FILTERED, F_INDEL_LEN, F_INDEL_KEY, F_ALT_COMMA = 1, 2, 4, 8, 16
INTERSECT, COMPLEMENT, CONCAT = 0, 1, 2
DROPPED, IGNORED, TAKEN, WRITTEN = 0, 1, 2, 3
HEADER = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"     # VCF_HEADER, vcf.c
MAX_LINE = 8190                 # LINE_BUF_SIZE 8192: fgets takes 8191 bytes, the '\n' among them
MAX_HEADER_LINES = 10000        # vcf.c:687


class Refused(Exception):
    def __init__(self, why, line, file=0):
        Exception.__init__(self, "refused: why %d at line %d of file %d" % (why, line, file))
        self.why, self.line, self.file = why, line, file


def split_lines(data):
    """[(start, bytes in front of the '\\n')]; a last line without '\\n' counts as if it had one"""
    out, at = [], 0
    while at < len(data):
        e = data.find(b"\n", at)
        e = len(data) if e < 0 else e
        out.append((at, data[at:e]))
        at = e + 1
    return out


def c_atol(tok, max_digits):
    """atol / atoi / strtol(.., 10): blanks, a sign, digits -> (value, more digits than max_digits)"""
    i = 0
    while i < len(tok) and tok[i:i + 1] in (b" ", b"\t", b"\n", b"\v", b"\f", b"\r"):
        i += 1
    neg = tok[i:i + 1] == b"-"
    if tok[i:i + 1] in (b"-", b"+"):
        i += 1
    j = i
    while j < len(tok) and 0x30 <= tok[j] <= 0x39:
        j += 1
    if j - i > max_digits:
        return 0, True
    v = int(tok[i:j]) if j > i else 0
    return (-v if neg else v), False


def int32(v):
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)


def info_key(info, key):
    """vcf_var_has_info_key (vcf.c:343-390) -> (found, value or None)"""
    if len(info) < 2:
        return False, None
    for tok in info.split(b";"):
        if len(tok) >= len(key) and tok[:len(key)].upper() == key.upper() and (len(tok) == len(key) or tok[len(key):len(key) + 1] == b"="):
            eq = tok.find(b"=")
            return True, (tok[eq + 1:] if eq >= 0 else None)
    return False, None


class Rec:
    """one record as vcf_parse_var_from_line (vcf.c:739-810) leaves it"""

    def __init__(self, line_no, text):
        text = text.rstrip(b"\r\n")                         # chomp, utils.c:487-497
        f = text.split(b"\t")                               # strsep: empty fields are fields
        self.line, self.n_fields_all = line_no, len(f)
        self.nf = min(len(f), 10)
        starts, at = [], 0
        for x in f:
            starts.append(at)
            at += len(x) + 1
        self.off = [starts[j] if j < self.nf else len(text) + 1 for j in range(9)] + [len(text)]
        self.hash = text[:1] == b"#"
        self.number = False
        self.chrom = f[0]
        self.pos, self.qual = -1, -1
        if len(f) >= 2:
            v, many = c_atol(f[1], 18)
            self.pos, self.number = v - 1, self.number or many
        self.id, self.ref, self.alt = (f + [b"", b"", b"", b""])[2:5]
        if len(f) >= 6 and f[5][:1] != b".":
            v, many = c_atol(f[5], 9)
            self.qual, self.number = v, self.number or many
        self.filter, self.info = (f[6], f[7]) if len(f) >= 8 else (b".", b".")
        self.rest = b"\t".join(f[8:]) if len(f) >= 9 else None      # FORMAT and the samples, verbatim
        self.flags = 0
        if len(f) >= 5:
            if self.filter[:1] == b"." or self.filter[:4] == b"PASS":           # VCF_VAR_PASSES, vcf.h:87
                self.flags |= F_PASSES
            if self.filter not in (b".", b"PASS"):                              # vcf_var_filtered, vcf.c:315-326
                self.flags |= F_FILTERED
            if len(self.ref) > 1 or len(self.alt) > 1:                          # vcf_var_is_indel, vcf.c:328-337
                self.flags |= F_INDEL_LEN
            if info_key(self.info, b"INDEL")[0]:
                self.flags |= F_INDEL_KEY
            if b"," in self.alt:
                self.flags |= F_ALT_COMMA
        elif len(f) < 8:
            self.flags |= F_PASSES

    @property
    def is_indel(self):
        return bool(self.flags & (F_INDEL_LEN | F_INDEL_KEY))

    def written(self, add=b""):
        """vcf_write_var (vcf.c:469-497) after vcf_var_add_to_info (vcf.c:500-521)"""
        info = self.info
        if add:
            info = add if info in (b".", b"") else info + b";" + add
        out = self.chrom + b"\t%d\t" % (self.pos + 1) + self.id + b"\t" + self.ref + b"\t" + self.alt + b"\t"
        out += (b"%d" % self.qual if self.qual > -1 else b".") + b"\t" + self.filter + b"\t" + info
        if self.rest is not None:
            out += b"\t" + self.rest
        return out + b"\n"


class Parsed:
    pass


def parse(data, mode=STREAM):
    data = bytes(data)
    p = Parsed()
    p.data, p.mode, p.lines = data, mode, split_lines(data)
    bad = []
    for k, (s, text) in enumerate(p.lines):
        if b"\0" in text:
            bad.append((k, NUL))
        if len(text) > MAX_LINE:
            bad.append((k, LINE_TOO_LONG))
    long_ = {k for k, why in bad if why == LINE_TOO_LONG}
    p.hdr_line, p.header = -1, b""
    if mode == STREAM:                                      # vcf_parse_header, vcf.c:684-720
        for k, (s, text) in enumerate(p.lines[:MAX_HEADER_LINES]):
            if text[:len(HEADER)] == HEADER:
                p.hdr_line = k
                p.header = data[:min(s + len(text) + 1, len(data))]
                break
        p.recs = []
        k = p.hdr_line + 1
        while k < len(p.lines) and k not in long_:
            r = Rec(k, p.lines[k][1])
            if r.n_fields_all < 5:                          # every caller's loop stops here
                break
            p.recs.append(r)
            k += 1
        p.behind = len(p.lines) - k
    else:
        p.recs, p.behind = [], 0
        for k, (s, text) in enumerate(p.lines):
            if text[:1] == b"#" or k in long_:
                continue
            r = Rec(k, text)
            if r.n_fields_all < 5:
                bad.append((k, FIELDS))
                continue
            p.recs.append(r)
    p.runs = []                                             # [(name, first record)]
    for i, r in enumerate(p.recs):
        if r.number:
            bad.append((r.line, NUMBER))
        head = i == 0 or p.recs[i - 1].chrom != r.chrom
        if head:
            p.runs.append((r.chrom, i))
        r.run = len(p.runs) - 1
        if mode == TABIX:
            found, end = info_key(r.info, b"END")
            end_bad = False
            if found and end is not None:
                v, many = c_atol(end, 18)
                end_bad = not many and v < r.pos + 1
            if r.pos < 0 or len(r.ref) < 1 or end_bad:
                bad.append((r.line, INTERVAL))
            if not head and r.pos < p.recs[i - 1].pos:
                bad.append((r.line, UNSORTED))
    if mode == TABIX and not bad:
        seen = set()
        for name, first in p.runs:
            if name in seen:
                bad.append((p.recs[first].line, UNSORTED))
            seen.add(name)
    if bad:
        k, why = min(bad)
        raise Refused(why, k + 1)
    return p


def table(p):
    """what lfq_vcf_records hands out and the check program prints: [line, pos, qual, flags, nf, off]"""
    return [[r.line, r.pos, r.qual, r.flags, r.nf, r.off] for r in p.recs]


def info_values(r):
    """[dp, sb, alt_fw, alt_rv, the bytes of AF's value or None] (vcf_get_dp4: vcf.c:566-604)"""
    out = []
    for key in (b"DP", b"SB"):
        found, v = info_key(r.info, key)
        out.append(int32(c_atol(v, 18)[0]) if found and v is not None else 0)
    found, v = info_key(r.info, b"DP4")
    f = v.split(b",") if found and v is not None else []
    out += [int32(c_atol(f[2], 18)[0]), int32(c_atol(f[3], 18)[0])] if len(f) == 4 else [-1, -1]
    found, v = info_key(r.info, b"AF")
    out.append(v if found and v is not None else None)
    return out


def c_strtof(text):
    """the C library's strtof, through the interpreter's own float parser on the longest numeric prefix, rounded once to float:
    valid for the decimal texts the tests use (no hex floats, no denormal double rounding)"""
    import re
    m = re.match(rb"[ \t\n\v\f\r]*([+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?))", text)
    return struct.unpack("f", struct.pack("f", float(m.group(1))))[0] if m else 0.0


def filter_vars(p):
    out = []
    for r in p.recs:
        dp, sb, fw, rv, af = info_values(r)
        out.append((int(r.is_indel), r.qual, dp, sb, fw, rv, c_strtof(af) if af is not None else 0.0))
    return out


def uniq_variants(p, chrom, only_unfiltered, uni_freq):
    """-> [(line, pos, ref, alt, indel_key, af)], or raises Refused(0, line) for a record without AF when uni_freq <= 0"""
    out = []
    for r in p.recs:
        if r.chrom != chrom or (only_unfiltered and r.flags & F_FILTERED):
            continue
        af = info_values(r)[4]
        if not uni_freq > 0 and af is None:
            raise Refused(OK, r.line + 1)
        out.append((r.line, r.pos, r.ref, r.alt, int(bool(r.flags & F_INDEL_KEY)), uni_freq if uni_freq > 0 else c_strtof(af)))
    return out


def bed_overlap(bed, beg, end):
    return any(e > beg and b < end for b, e in bed)


def ign_mask(p, chrom, ref_len, bed=None):
    """source_qual_load_ign_vcf (plp.c:337-399) -> the positions set"""
    return sorted({r.pos for r in p.recs if r.chrom == chrom and 0 <= r.pos < ref_len and (bed is None or bed_overlap(bed, r.pos, r.pos + 1))})


def vcfset(ones, two, op=INTERSECT, only_passed=0, only_pos=0, only_snvs=0, only_indels=0, count_only=0, add=b""):
    """lofreq_vcfset.c:346-508 over parsed files: `ones` is [file 1] (+ the further files of concat), `two` file 2 in tabix mode"""
    keep, lines, bad = [], [], []
    by_chrom = {}
    if op != CONCAT:
        for r in two.recs:
            by_chrom.setdefault((r.chrom, r.pos), []).append(r)
    for fi, one in enumerate(ones if op == CONCAT else ones[:1]):
        for r in one.recs:
            if (only_snvs and r.is_indel) or (only_indels and not r.is_indel):              # :387-394
                keep.append(DROPPED)
                continue
            if not only_pos and r.flags & F_ALT_COMMA:                                      # :396-399
                bad.append((fi, r.line, MULTIALLELIC))
                keep.append(DROPPED)
                continue
            if only_passed and not r.flags & F_PASSES:                                      # :400-407
                keep.append(IGNORED)
                continue
            if op == CONCAT:
                match = True
            else:
                if r.pos < 0:
                    bad.append((fi, r.line, INTERVAL))
                    keep.append(TAKEN)
                    continue
                hit = False
                for c in by_chrom.get((r.chrom, r.pos), []):                                # :452-477
                    if only_passed and not c.flags & F_PASSES:
                        continue
                    if (only_snvs and c.is_indel) or (only_indels and not c.is_indel):
                        continue
                    if only_pos or (c.ref == r.ref and c.alt == r.alt):
                        hit = True
                        break
                match = hit == (op == INTERSECT)
            keep.append(WRITTEN if match else TAKEN)
            if match:
                lines.append(r.written(add))
    if bad:
        fi, line, why = min(bad)
        raise Refused(why, line + 1, fi)
    text = b"" if count_only else (ones[0].header if ones[0].hdr_line >= 0 else b"") + b"".join(lines)
    return {"counts": (sum(k >= TAKEN for k in keep), keep.count(IGNORED), keep.count(WRITTEN)), "keep": keep, "text": text}
