"""`lofreq faidx` and the whole-contig fetch restated in Python, a byte at a time as htslib's fai_build_core and fai_retrieve walk
the file (the 2.1.4 binary's behaviour: tests/golden/fasta_binary.json holds this model to it, tests/test_fasta_model.py).  The
library states the same rules per line (lofreq_amd/csrc/lfq_fasta.h); the tests hold both to this one.

    build(data)  -> {"status": 0, "fai": bytes, "entries": [(name, length, offset, line_blen, line_len)], "n_dup": k, "log": [...]}
                    {"status": 1, "why": UNEXPECTED | LINE_LENGTH | LAST_EMPTY | EMPTY_FILE, "line": N, "byte": b, "log": [...]}
    fetch(data, entry) -> bytes, or None when fewer than `length` graph bytes stand at or behind `offset`
    gzi(comp_off, data_off) -> the .gzi bytes of a BGZF file from its block tables
    checkref(entries, names, lens) -> (first_bad, why)
"""
import struct

UNEXPECTED, LINE_LENGTH, LAST_EMPTY, EMPTY_FILE = 1, 2, 3, 4
NO_SEQUENCE, LENGTH = 1, 2
_SPACE = b" \t\n\v\f\r"


def isgraph(c):
    return 0x21 <= c <= 0x7e


def build(data):
    data = bytes(data)
    n = len(data)
    log, entries, names, n_dup = [], [], set(), 0
    OUT, NAME, SEQ = 0, 1, 2
    state, i, line = OUT, 0, 1
    name, seq_len, line_len, char_len, seq_off, read_done = b"", 0, 0, 0, 0, False

    def fail(why, ln, byte, msg=None):
        if msg:
            log.append(msg)
        return {"status": 1, "why": why, "line": ln, "byte": byte, "log": log}

    def insert():
        nonlocal n_dup
        if name in names:
            log.append('Ignoring duplicate sequence "%s" at byte offset %d' % (name.decode("latin-1"), seq_off))
            n_dup += 1
        else:
            names.add(name)
            entries.append((name, seq_len, seq_off, char_len, line_len))

    while i < n:
        c = data[i]
        i += 1
        if state == OUT:
            if c == 0x3e:
                state = NAME
            elif c == 0x0a:
                line += 1
            elif c == 0x0d:
                if i < n and data[i] == 0x0a:
                    i += 1
                    line += 1
                else:
                    return fail(UNEXPECTED, line, data[i] if i < n else -1,
                                "Format error, carriage return not followed by new line at line %d" % line)
            else:
                return fail(UNEXPECTED, line, c, 'Format error, unexpected "%c" at line %d' % (c, line) if 0x20 <= c <= 0x7e
                            else "Format error, unexpected character at line %d" % line)
        elif state == NAME:
            if read_done:
                insert()
                read_done = False
            nm = bytearray()
            while True:
                if c not in _SPACE:
                    nm.append(c)
                elif nm or c == 0x0a:
                    break
                if i >= n:
                    c = -1
                    break
                c = data[i]
                i += 1
            name = bytes(nm)
            if c < 0:
                return fail(LAST_EMPTY, 0, 0, "The last entry '%s' has no sequence" % name.decode("latin-1"))
            while c != 0x0a:
                if i >= n:
                    c = -1
                    break
                c = data[i]
                i += 1
            state = SEQ
            seq_len = line_len = char_len = 0
            seq_off = i
            line += 1
        else:
            if c == 0x0a:
                state = OUT
                line += 1
                continue
            if c == 0x3e:
                state = NAME
                continue
            ll = cl = 0
            c0 = c
            read_done = True
            while True:
                ll += 1
                cl += isgraph(c)
                if i >= n:
                    break
                c = data[i]
                i += 1
                if c == 0x0a:
                    break
            ll += 1
            seq_len += cl
            if line_len == 0:
                line_len, char_len = ll, cl
            elif line_len > ll:
                state = OUT
            elif line_len < ll:
                return fail(LINE_LENGTH, line, c0, "Different line length in sequence '%s'" % name.decode("latin-1"))
            line += 1
    if not read_done:
        return fail(LAST_EMPTY if _has_header(data) else EMPTY_FILE, 0, 0)
    insert()
    fai = b"".join(e[0] + b"\t%d\t%d\t%d\t%d\n" % e[1:] for e in entries)
    return {"status": 0, "fai": fai, "entries": entries, "n_dup": n_dup, "log": log}


def _has_header(data):
    return data.startswith(b">") or b"\n>" in data


def fetch(data, entry):
    _, length, offset = entry[:3]
    if offset < 0 or offset > len(data) or length < 0:
        return None
    out = bytearray()
    i = offset
    while len(out) < length and i < len(data):
        if isgraph(data[i]):
            out.append(data[i])
        i += 1
    return bytes(out) if len(out) == length else None


def is_regular(data, entry):
    """the library's proof: every line of the span but the last is line_blen graph bytes and '\\n'"""
    _, length, offset, blen, llen = entry
    if length == 0 or blen <= 0 or llen != blen + 1:
        return False
    for p in range(length):
        s = offset + p // blen * llen + p % blen
        if s >= len(data) or not isgraph(data[s]):
            return False
    for k in range((length + blen - 1) // blen):
        s = offset + k * llen
        if s > 0 and data[s - 1] != 0x0a:
            return False
        if k < (length + blen - 1) // blen - 1 and data[s + blen:s + blen + 1] != b"\n":
            return False
    return True


def parse_fai(text):
    out = []
    for ln in bytes(text).split(b"\n"):
        if ln:
            f = ln.split(b"\t")
            out.append((f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4])))
    return out


def gzi(comp_off, data_off):
    """htslib's reader, one entry per read call: it skips empty blocks until one holds data and records where the call began; the
    first entry (0, 0) is not written"""
    pairs, prev, first = [], -1, True
    for b in range(len(comp_off) - 1):
        if data_off[b + 1] > data_off[b]:
            if not first:
                pairs.append((comp_off[prev + 1], data_off[b]))
            first, prev = False, b
    return struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", a, b) for a, b in pairs)


def checkref(entries, names, lens):
    by = {}
    for e in entries:
        by.setdefault(bytes(e[0]), e[1])
    for i, (nm, ln) in enumerate(zip(names, lens)):
        nm = nm.encode("latin-1") if isinstance(nm, str) else bytes(nm)
        if nm not in by:
            return i, NO_SEQUENCE
        if by[nm] != ln:
            return i, LENGTH
    return -1, 0
