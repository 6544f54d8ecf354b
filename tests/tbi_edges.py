"""Small inputs of lfq_vcf_index_build placed on its constants: one table for the Python model (tests/tbi_model.py), for the host program
(tests/test_tbi_edges.py), for the device (tests/test_gpu_vcf_index.py) and -- the BINARY rows -- for the reference's 2.1.4 binary
(tests/make_tbi_golden.py -> tests/golden/tbi_binary.json).

  ROWS     a row is a tabix-mode VCF text and a FABRICATED block table -- the builder takes the tables as arguments, so nothing has to
           be compressed, a block can end anywhere in a line and a compressed span can be put on 65536 at will.  `refused`: None, or
           (why, 1-based line).  What the index of a row is comes from tbi_model.build.
  BINARY   texts `lofreq filter --no-defaults -o x.vcf.gz` is run over: what the binary writes is the fixture's, its blocks included.
           Every line stays below the 4 095 bytes behind which the binary splits a line.
  PARSE    byte strings lfq_vcf_index_parse refuses, made from a good .tbi.
No test in here."""
import collections
import struct

import bam_records as br
import tbi_model as tm
import vcf_model as vm

WG = br.source_constant("LFQ_BAI_THREADS", "lofreq_amd/csrc/lfq_bamidx.hip")       # a workgroup of the compaction kernels
TBX_WG = br.source_constant("LFQ_TBX_THREADS", "lofreq_amd/csrc/lfq_tbx.hip")      # a workgroup of the record kernel
WAVE = 64
ROUND = 64 * WG                 # records a round of lfq_bai_scan_kernel covers: 64 parts of a workgroup each
W = 1 << 14
LIMIT = 1 << 29
HEAD = b"##fileformat=VCFv4.0\n" + vm.HEADER + b"\n"

Row = collections.namedtuple("Row", "name text data_off comp_off file_off refused")
ROWS, BINARY, PARSE = [], [], []


def rec(chrom=b"c1", pos=1, ref=b"A", alt=b"C", info=b"DP=9"):
    return b"%s\t%d\t.\t%s\t%s\t50\tPASS\t%s\n" % (chrom, pos, ref, alt, info)


def tables(n, piece, comp=None):
    """n bytes cut every `piece` bytes (or at the list `piece` of sizes); compressed sizes `comp` (a number, a list; default 90 + 7 b)"""
    sizes = piece if isinstance(piece, list) else [min(piece, n - a) for a in range(0, n, piece)]
    assert sum(sizes) == n, (sum(sizes), n)
    data_off, comp_off = [0], [0]
    for b, s in enumerate(sizes):
        data_off.append(data_off[-1] + s)
        comp_off.append(comp_off[-1] + (comp if isinstance(comp, int) else comp[b] if comp else 90 + 7 * (b % 13)))
    return data_off, comp_off


def row(name, text, piece=1000, comp=None, file_off=0, refused=None):
    d, c = tables(len(text), piece, comp)
    ROWS.append(Row(name, text, d, c, file_off, refused))


def run_of(n, chrom=b"c1", first=1, step=3):
    return b"".join(rec(chrom, first + step * i) for i in range(n))


# ---- record counts: the wavefront, the workgroups of both kernels, one round of the scan kernel and more ------------------------------
COUNTS = sorted({1, WAVE - 1, WAVE, WAVE + 1, WG - 1, WG, WG + 1, TBX_WG - 1, TBX_WG, TBX_WG + 1, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 5})
for n in COUNTS:
    row("%d_records" % n, HEAD + run_of(n, step=37), piece=4099)       # (37: windows, and with them chunks, change along the run)

# ---- block boundaries ---------------------------------------------------------------------------------------------------------------
_t = HEAD + run_of(5)
_ln = [s for s, _ in vm.split_lines(_t)]
row("line_starts_a_block", _t, piece=[_ln[3], len(_t) - _ln[3]])
row("line_straddles_two_blocks", _t, piece=[_ln[3] + 4, len(_t) - _ln[3] - 4])
row("line_across_three_blocks", _t, piece=[_ln[3] + 2, 3, len(_t) - _ln[3] - 5])
row("empty_block_between", _t, piece=[_ln[3], 0, len(_t) - _ln[3]])
row("header_alone_in_the_first_block", _t, piece=[len(HEAD), len(_t) - len(HEAD)])
row("one_block", _t, piece=[len(_t)])
row("a_block_per_line", _t, piece=[b - a for a, b in zip(_ln, _ln[1:] + [len(_t)])])
row("file_off_above_zero", _t, piece=50, file_off=123456789)
row("no_newline_at_the_end", _t[:-1], piece=50)
row("marker_blocks_in_the_tables", _t, piece=[100, len(_t) - 100, 0, 0])
# rule 6: bin 4682's first and last chunk lie 65 535 / 65 536 compressed bytes apart, and its parent 585 is there (the long REF)
_wide = HEAD + rec(pos=5) + rec(pos=W, ref=b"AC") + rec(pos=W + 5) + rec(pos=W + 6) + rec(pos=W + 7) + rec(pos=W + 8)
_wl = [s for s, _ in vm.split_lines(_wide)]
for span in (65535, 65536):
    row("wide_bin_span_%d" % span, _wide, piece=[_wl[2]] + [b - a for a, b in zip(_wl[2:], _wl[3:] + [len(_wide)])],
        comp=[100, 100, 100, 100, span - 300, 100, 100])

# ---- intervals ----------------------------------------------------------------------------------------------------------------------
row("ref_across_a_window_edge", HEAD + rec(pos=W - 1, ref=b"ACG") + rec(pos=W, ref=b"AC") + rec(pos=W + 1) + rec(pos=2 * W, ref=b"A" * 300))
for lvl, shift in ((4, 17), (3, 20), (2, 23), (1, 26)):
    e = 3 << shift
    row("ref_across_a_level_%d_edge" % lvl, HEAD + rec(pos=e - 1) + rec(pos=e, ref=b"AC") + rec(pos=e, ref=b"A") + rec(pos=e + 1))
row("end_keys", HEAD + rec(pos=5, info=b"END=5") + rec(pos=6, info=b"END=400000;DP=1") + rec(pos=7, info=b"DP=1;END=400000")
    + rec(pos=8, info=b"DP=1;end=20000") + rec(pos=9, info=b"END") + rec(pos=10, info=b"END=70000x") + rec(pos=11, info=b"XEND=99999;ENDX=5"))
row("end_key_no_number", HEAD + rec(pos=8, info=b"END=x9"), refused=(vm.INTERVAL, 3))
row("equal_pos_runs_of_1_2_65", HEAD + rec(pos=4) + rec(pos=9) + rec(pos=9, alt=b"G") + b"".join(rec(pos=W + 3, alt=b"G" * (1 + i)) for i in range(65)),
    piece=77)
row("pos_and_end_at_the_limit", HEAD + rec(pos=LIMIT - 1) + rec(pos=LIMIT - 1, ref=b"AC") + rec(pos=LIMIT) + rec(b"c2", 5, info=b"END=%d" % LIMIT))
row("pos_one_above_the_limit", HEAD + rec(pos=LIMIT) + rec(pos=LIMIT + 1), refused=(tm.RANGE, 4))
row("pos_five_above_the_limit", HEAD + rec(pos=LIMIT + 5), refused=(tm.RANGE, 3))
row("ref_runs_over_the_limit", HEAD + rec(pos=LIMIT, ref=b"AC"), refused=(tm.RANGE, 3))
row("end_one_above_the_limit", HEAD + rec(pos=5, info=b"END=%d" % (LIMIT + 1)), refused=(tm.RANGE, 3))
row("end_of_19_digits", HEAD + rec(pos=5, info=b"END=1000000000000000000"), refused=(tm.RANGE, 3))

# ---- CHROM runs ---------------------------------------------------------------------------------------------------------------------
for edge in (1, WAVE, WG, TBX_WG):
    row("run_boundary_at_record_%d" % edge, HEAD + run_of(edge, b"c1") + run_of(WG + 3, b"c2"), piece=997)
row("a_run_of_one_record", HEAD + run_of(3, b"c1") + rec(b"c2", 77) + run_of(3, b"c3"))
row("more_names_than_a_workgroup_has_lanes", HEAD + b"".join(rec(b"n%d" % i, 1 + i % 5) for i in range(TBX_WG + WG + 7)), piece=313)

# ---- '#' lines ----------------------------------------------------------------------------------------------------------------------
row("hash_in_front", HEAD + b"#late\tx\n" + run_of(3), piece=40)
row("hash_between_records_of_a_run", HEAD + rec(pos=1) + b"#late\n" + rec(pos=W + 1) + b"##x\ty\n#z\n" + rec(pos=2 * W + 1), piece=40)
row("hash_between_runs", HEAD + rec(pos=1) + b"#late\n" + rec(b"c2", 1) + rec(b"c2", 2), piece=40)
row("hash_at_the_end", HEAD + rec(pos=1) + rec(pos=W + 2) + b"#late\n##x\n", piece=40)
row("hash_anywhere", HEAD + rec(pos=1) + b"#late\n" + rec(pos=1, alt=b"G") + rec(b"c2", 1) + b"##x\ty\n", piece=33)

# ---- refusals in the first, a middle and the last workgroup ------------------------------------------------------------------------------
_N = 3 * TBX_WG + 10
for where, at in (("first", 5), ("middle", TBX_WG + WG + 9), ("last", _N - 1)):
    good = [rec(pos=1 + 3 * i) for i in range(_N)]
    # the offender and two more behind it (the FIRST line is reported); what follows is another name's, so the file stays sorted
    lines = good[:at] + [rec(pos=LIMIT + 1 + i) for i in range(at, min(at + 3, _N))] + [rec(b"c2", 1 + 3 * i) for i in range(at + 3, _N)]
    row("range_in_the_%s_workgroup" % where, HEAD + b"".join(lines), piece=4099, refused=(tm.RANGE, 3 + at))
    for why, bad in ((vm.UNSORTED, rec(pos=1)), (vm.FIELDS, b"c1\t5\t.\tA\n"), (vm.INTERVAL, rec(pos=1 + 3 * at, ref=b""))):
        if why == vm.UNSORTED and at == 0:
            continue
        row("open_refuses_%d_in_the_%s_workgroup" % (why, where), HEAD + b"".join(good[:at] + [bad] + good[at + 1:]), piece=4099,
            refused=(why, 3 + at))

# ---- no records -----------------------------------------------------------------------------------------------------------------------
row("header_only", HEAD, piece=[len(HEAD)])
row("empty", b"", piece=[])

# ---- the binary's rows --------------------------------------------------------------------------------------------------------------------
_big = [rec(b"c1", 1 + 61 * i, info=b"DP=%d;AF=0.01" % i) for i in range(1500)]
_big[700] = rec(b"c1", 1 + 61 * 700, ref=b"ACGT" * 750)                          # 3 000 bytes of REF, across a window edge
_big[5] = rec(b"c1", 1 + 61 * 5, info=b"END=400000;DP=1")
_big[9] = rec(b"c1", 1 + 61 * 9, info=b"DP=1;END=400000")
_big += [rec(b"c2", 1 + 977 * i) for i in range(1200)] + [rec(b"c3", LIMIT - 1), rec(b"c3", LIMIT)]
BINARY += [
    ("three_runs_many_blocks", HEAD + b"".join(_big)),
    ("one_record", HEAD + rec(pos=5)),
    ("bin_level_edges", HEAD + b"".join(rec(pos=(3 << s) + d, ref=r) for s in (14, 17, 20, 23, 26) for d, r in ((-1, b"A"), (0, b"AC"), (0, b"A"), (1, b"A")))),
    ("end_keys", [r for r in ROWS if r.name == "end_keys"][0].text),
    ("equal_pos_runs_of_1_2_65", [r for r in ROWS if r.name == "equal_pos_runs_of_1_2_65"][0].text),
    ("many_names", [r for r in ROWS if r.name == "more_names_than_a_workgroup_has_lanes"][0].text),
    ("pos_and_end_at_the_limit", [r for r in ROWS if r.name == "pos_and_end_at_the_limit"][0].text),
    ("pos_one_above_the_limit", [r for r in ROWS if r.name == "pos_one_above_the_limit"][0].text),
    ("pos_five_above_the_limit", [r for r in ROWS if r.name == "pos_five_above_the_limit"][0].text),
    ("end_one_above_the_limit", [r for r in ROWS if r.name == "end_one_above_the_limit"][0].text),
    # `filter` reads a '#' line behind the header as a record and writes it through; tbx_index_build then skips it as a meta line
    ("hash_in_front", HEAD + rec(b"#c1", 6) + run_of(3)),
    ("hash_between_records_of_a_run", HEAD + rec(pos=1) + rec(b"#c1", 6) + rec(pos=W + 1) + rec(b"#x", 1) + rec(b"#y", 1) + rec(pos=2 * W + 1)),
    ("hash_between_runs", HEAD + rec(pos=1) + rec(b"#late", 9) + rec(b"c2", 1) + rec(b"c2", 2)),
    ("hash_at_the_end", HEAD + rec(pos=1) + rec(pos=W + 2) + rec(b"#late", 1) + rec(b"#x", 2)),
    ("file_twice", HEAD + (run_of(3, b"c1") + run_of(3, b"c2")) * 2),
    ("header_only", HEAD),
    ("empty", b""),
]


def queries(text):
    """[(name, beg, end)] worth asking of a row: at every run's first and last record, around a middle one, the whole name, an absent
    name, an empty region"""
    try:
        p = vm.parse(text, vm.TABIX)
    except vm.Refused:
        return []
    out = [(b"absent", 0, 100), (b"c1", 7, 7)]
    for i, (name, first) in enumerate(p.runs):
        last = (p.runs[i + 1][1] if i + 1 < len(p.runs) else len(p.recs)) - 1
        if i > 4 and i + 3 < len(p.runs):
            continue
        mid = p.recs[(first + last) // 2].pos
        out += [(name, p.recs[first].pos, p.recs[first].pos + 1), (name, p.recs[last].pos, p.recs[last].pos + 1), (name, 0, LIMIT),
                (name, max(mid - 5, 0), mid + 5), (name, mid + 1, mid + W)]
    return out


def expected(r):
    """-> tbi_model's parsed index of a row, or (why, line)"""
    try:
        return tm.build(r.text, r.data_off, r.comp_off, r.file_off)
    except vm.Refused as e:
        return (e.why, e.line)


# ---- parse refusals --------------------------------------------------------------------------------------------------------------------
def _parse_rows():
    good = tm.to_bytes(tm.build(HEAD + run_of(3, b"c1") + run_of(2, b"c22"), *tables(len(HEAD + run_of(3, b"c1") + run_of(2, b"c22")), 60)))
    l_nm = struct.unpack_from("<i", good, 32)[0]
    assert good[36:36 + l_nm] == b"c1\0c22\0"
    put = lambda at, v: good[:at] + struct.pack("<i", v) + good[at + 4:]
    return good, [
        ("no_magic", b"TBJ\1" + good[4:]),
        ("bai_magic", b"BAI\1" + good[4:]),
        ("too_short", good[:35]),
        ("n_ref_past_the_end", put(4, 1 << 20)),
        ("n_ref_negative", put(4, -1)),
        ("l_nm_past_the_end", put(32, len(good))),
        ("l_nm_negative", put(32, -7)),
        ("l_nm_one_short", put(32, l_nm - 1)),                  # the last name loses its NUL
        ("one_name_too_many", put(4, 1)),
        ("one_name_too_few", put(4, 3)),
        ("a_name_twice", good[:36] + b"c1\0c1\0\0" + good[36 + l_nm:]),
        ("n_bin_past_the_end", put(36 + l_nm, 1 << 20)),
        ("bytes_left_over", good + b"\0"),
        ("cut_in_a_chunk", good[:36 + l_nm + 20]),
    ]


GOOD_TBI, PARSE = _parse_rows()
