"""FASTA files placed on the boundaries of the scan, line, entry and fetch kernels of lofreq_amd/csrc/lfq_fasta.hip, for the check
program (tests/test_fasta_edges.py) and the device (tests/test_gpu_fasta.py).  The geometry is read from lfq_fasta.h: a lane owns a
CHUNK of 16 aligned bytes, a wavefront 64 of them, a workgroup a TILE of THREADS chunks, and the scan over the tiles' sums takes
SCAN_LANES tiles a round.  What a row must give comes from tests/fasta_model.py, never from the code under test.

    ROWS   [{"name", "data": bytes, "fai": None | bytes (a foreign .fai to fetch by), "where": {what the row promises: byte offsets}}]
"""
import numpy as np

import bam_records as br
import fasta_model as fm

_H = "lofreq_amd/csrc/lfq_fasta.h"
CHUNK = br.source_constant("LFQ_FA_CHUNK", _H)
THREADS = br.source_constant("LFQ_FA_THREADS", _H)
SCAN_LANES = br.source_constant("LFQ_FA_SCAN_LANES", _H)
WAVE = 64 * CHUNK
TILE = THREADS * CHUNK

_rng = np.random.default_rng(20261021)


def bases(n):
    return bytes(_rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), n).tolist())


def wrap(seq, w, eol=b"\n"):
    return b"".join(seq[i:i + w] + eol for i in range(0, len(seq), w))


def contig(name, n, w, eol=b"\n"):
    return b">" + name + eol + wrap(bases(n), w, eol)


def fill_to(buf, pos, name=b"fill", w=60):
    """buf + a contig of width w whose last byte, a '\n', is byte pos - 1 (where the room does not divide, a shorter last line; where
    one byte is left over, an empty line, which ends a sequence as well)"""
    head = b">" + name + b"\n"
    n_full, rest = divmod(pos - len(buf) - len(head), w + 1)
    assert n_full >= 1 or rest >= 2
    out = buf + head + wrap(bases(n_full * w), w) + (b"" if rest == 0 else bases(rest - 1) + b"\n")
    assert len(out) == pos and out[-1:] == b"\n"
    return out


ROWS = []


def row(name, data, fai=None, **where):
    ROWS.append({"name": name, "data": bytes(data), "fai": fai, "where": where})


# ---- line widths ----
for w in (1, 15, 16, 17, 60, 61, 63, 64, 65):
    row("width_%d" % w, contig(b"a", 37 * w + (w > 1) * (w // 2), w) + contig(b"b", 1500 + w, w))
row("width_wider_than_a_tile", contig(b"a", 2 * (TILE + 904) + 17, TILE + 904) + contig(b"b", 70, 60), wide=TILE + 904)

# ---- a '\n' as the last byte of a chunk, of a wavefront's span, of a tile; '>' as a tile's first byte ----
for what, edge in (("chunk", CHUNK), ("wave", WAVE), ("tile", TILE)):
    d = fill_to(b"", edge, b"e") + contig(b"next", 130, 60)
    row("newline_ends_%s" % what, d, newline=edge - 1, header=edge)
row("header_starts_tile", fill_to(b"", 2 * TILE) + contig(b"t", 200, 60), header=2 * TILE)

# ---- "\r\n" split across a tile; a header that straddles two tiles ----
d = b">c\r\n" + wrap(bases(TILE), 58, b"\r\n")
k = d.index(b"\r\n", TILE - 70)
d = b">c" + b"x" * (TILE - 1 - k) + d[2:]        # a longer name moves that '\r' to the tile's last byte
row("crlf_split_across_tile", d, cr=TILE - 1)
d = fill_to(b"", TILE - 9) + b">straddle  the rest of a header line\n" + wrap(bases(333), 60) + contig(b"z", 61, 60)
row("header_straddles_tiles", d, header=TILE - 9)

# ---- a file of one tile, one byte less, one byte more ----
row("file_one_tile", fill_to(b"", TILE), size=TILE)
row("file_one_tile_minus_1", fill_to(b"", TILE)[:-1], size=TILE - 1)          # ... and the last line has no '\n'
row("file_one_tile_plus_1", fill_to(b"", TILE - 3)[:-1] + b"\n>q\nA", size=TILE + 1)
row("file_one_chunk", b">c\n" + bases(12) + b"\n", size=CHUNK)
row("file_one_byte_sequence", b">c\nA", size=4)

# ---- more tiles than the scan takes in a round ----
row("scan_two_rounds", contig(b"big", (SCAN_LANES + 3) * TILE, 60) + contig(b"tail", 77, 60), tiles=SCAN_LANES + 3)

# ---- many sequences ----
row("thousand_one_base", b"".join(b">s%d\n%c\n" % (i, b"ACGT"[i % 4]) for i in range(1000)))

# ---- an irregular sequence (blanks inside lines, equal line bytes) and its regular twin ----
_s = bases(3 * TILE + 500)
_lines = [_s[i:i + 59] for i in range(0, len(_s), 59)]
_irr = b"".join((l[:j % 59] + b" " + l[j % 59:] if len(l) == 59 else l) + b"\n" for j, l in enumerate(_lines))
row("irregular_blanks", b">c1 irregular\n" + _irr + contig(b"c2", 100, 60), letters=_s, path="general")
row("regular_twin", b">c1 regular\n" + wrap(_s, 60) + contig(b"c2", 100, 60), letters=_s, path="regular")
row("crlf_takes_general", contig(b"c1", 1000, 60, b"\r\n"), path="general")

# ---- endings ----
row("last_line_without_newline", contig(b"a", 290, 60)[:-1])
row("last_line_without_newline_full", contig(b"a", 300, 60)[:-1])
row("trailing_empty_lines", contig(b"a", 290, 60) + b"\n\n\r\n\n")

# ---- sequences without a line: at the start, in the middle, in front of a tile edge ----
row("dropped_at_start", b">none\n" + contig(b"a", 100, 60))
row("dropped_in_middle", contig(b"a", 100, 60) + b">none\n\n\n" + contig(b"b", 100, 60) + b">none2\n" + contig(b"c", 10, 60))
row("dropped_at_tile_edge", fill_to(b"", TILE - 6) + b">none\n" + contig(b"b", 100, 60), header=TILE - 6)

# ---- each refusal with its offending line in the first, a middle and the last tile ----
_three = [fill_to(b"", TILE, b"t0"), fill_to(b"", TILE, b"t1"), fill_to(b"", TILE, b"t2")]
_bad = {"unexpected": b">u\nACGT\nAC\nACGT\n", "line_length": b">l\nACGT\nACGTAC\n", "cr_alone": b">r\nACGT\nAC\n\rX\n"}
for what, text in _bad.items():
    row("%s_in_first_tile" % what, text + b"".join(_three), refused=True)
    row("%s_in_middle_tile" % what, _three[0] + text + _three[1] + _three[2], refused=True)
    row("%s_in_last_tile" % what, b"".join(_three) + text, refused=True)
row("last_entry_empty", b"".join(_three) + b">last\n", refused=True)
row("last_entry_empty_no_newline", b"".join(_three) + b">last", refused=True)
row("text_before_first_header", b"ACGT\n" + b"".join(_three), refused=True)
row("no_header_at_all", b"\n" * (TILE + 5), refused=True)
# two offending lines in different tiles: the earlier one is the answer, whichever lane gets there first
row("two_offences", _three[0] + _bad["line_length"] + _three[1] + _bad["unexpected"] + _three[2], refused=True)
row("two_offences_other_order", _three[0] + _bad["unexpected"] + _three[1] + _three[2] + _bad["line_length"], refused=True)

# ---- a parsed index: one that another tool made for these bytes, a stale one that still fits, one that runs past the file ----
_d = contig(b"a", 500, 60) + contig(b"b", 200, 50)
row("foreign_index_fits", _d, fai=b"a\t500\t3\t60\t61\nb\t200\t515\t50\t51\n")
row("foreign_index_stale_fits", _d, fai=b"a\t300\t10\t70\t71\nb\t100\t400\t50\t51\nwhole\t700\t0\t60\t61\n")
row("foreign_index_runs_past", _d, fai=b"a\t500\t3\t60\t61\nb\t260\t515\t50\t51\nfar\t1\t%d\t1\t2\n" % (len(_d) + 1))
row("foreign_index_offset_at_end", _d, fai=b"a\t500\t3\t60\t61\nend\t0\t%d\t1\t2\nend1\t1\t%d\t1\t2\n" % (len(_d), len(_d)))


def expected(r):
    """-> the model's answer for a row: build(data), and per entry of the index to fetch by (name, bytes | None, regular?)"""
    m = fm.build(r["data"])
    entries = fm.parse_fai(r["fai"]) if r["fai"] is not None else m.get("entries", [])
    return m, [(e, fm.fetch(r["data"], e), fm.is_regular(r["data"], e)) for e in entries]
