"""VCF files placed on the boundaries of the kernels of lofreq_amd/csrc/lfq_vcf.hip, and the cases `lofreq vcfset` is defined by, for
the check program (tests/test_vcf_edges.py) and the device (tests/test_gpu_vcf.py).  The geometry is read from lfq_vcf.hip: a lane owns
a CHUNK of 16 aligned bytes, a wavefront 64 of them, a workgroup a TILE, and the scan over the tiles' sums takes SCAN_LANES tiles a
round.  What a row must give comes from tests/vcf_model.py, never from the code under test.

    OPEN   [{"name", "mode", "data", "where": {what the row promises}}]
    SETS   [{"name", "conf": {op, only_passed, only_pos, only_snvs, only_indels, count_only, add}, "one", "two", "more", "where"}]
    MASKS  [{"name", "data", "chrom", "ref_len", "bed": None | [(beg, end)]}]
"""
import bam_records as br
import vcf_model as vm

_K = "lofreq_amd/csrc/lfq_vcf.hip"
CHUNK = br.source_constant("LFQ_VCF_CHUNK", _K)
THREADS = br.source_constant("LFQ_VCF_THREADS", _K)
TILE = br.source_constant("LFQ_VCF_TILE", _K)
SCAN_LANES = br.source_constant("LFQ_VCF_SCAN_LANES", _K)
WAVE = 64 * CHUNK
LIST_ROUND = br.source_constant("LFQ_VCF_SCAN_THREADS", _K) * br.source_constant("LFQ_VCF_SCAN_ITEMS", _K)

META = b"##fileformat=VCFv4.0\n"
HEAD = META + vm.HEADER + b"\n"
INFO = b"DP=100;AF=0.050000;SB=3;DP4=50,45,3,2"


def rec(chrom=b"c1", pos=1, ref=b"A", alt=b"C", qual=b"50", flt=b"PASS", info=INFO, vid=b".", extra=()):
    pos = pos if isinstance(pos, bytes) else b"%d" % pos
    return b"\t".join([chrom, pos, vid, ref, alt, qual, flt, info] + list(extra)) + b"\n"


def comment_to(buf, pos):
    """buf + '##' lines whose last byte, a '\\n', is byte pos - 1"""
    while len(buf) < pos:
        room = pos - len(buf)
        n = room if room <= 203 else 200
        assert n >= 3
        buf += b"##" + b"x" * (n - 3) + b"\n"
    assert len(buf) == pos
    return buf


def records_to(buf, pos, chrom=b"c1", first=1):
    """buf + records of `chrom` at first, first + 1, .. whose last byte is byte pos - 1 (the last one's INFO is padded)"""
    p = first
    while True:
        r = rec(chrom, p)
        if len(buf) + 2 * len(r) + 8 > pos:
            break
        buf += r
        p += 1
    room = pos - len(buf) - len(rec(chrom, p, info=b"DP=1;X="))
    assert room >= 0
    buf += rec(chrom, p, info=b"DP=1;X=" + b"x" * room)
    assert len(buf) == pos
    return buf, p + 1


OPEN, SETS, MASKS = [], [], []


def open_row(name, data, mode=vm.STREAM, **where):
    OPEN.append({"name": name, "mode": mode, "data": bytes(data), "where": where})


def set_row(name, one, two=None, more=(), where=None, **conf):
    c = {"op": vm.INTERSECT, "only_passed": 0, "only_pos": 0, "only_snvs": 0, "only_indels": 0, "count_only": 0, "add": b""}
    c.update(conf)
    SETS.append({"name": name, "conf": c, "one": bytes(one), "two": None if two is None else bytes(two), "more": [bytes(m) for m in more],
                 "where": where or {}})


# ---- the rules, small ------------------------------------------------------------------------------------------------------------------
MIXED = HEAD + b"".join([
    rec(pos=b"007"), rec(pos=b"12abc", qual=b"37.9"), rec(pos=13, qual=b".5"), rec(pos=14, qual=b"."), rec(pos=15, qual=b""),
    rec(pos=16, flt=b"PASSx"), rec(pos=17, flt=b".x"), rec(pos=18, flt=b"q20"), rec(pos=19, flt=b"."), rec(pos=20, flt=b""),
    rec(pos=21, info=b"INDEL;DP=5"), rec(pos=22, info=b"DP=5;indel=1"), rec(pos=23, info=b"XINDEL;DP=7"), rec(pos=24, info=b"DP=5;INDELX"),
    rec(pos=25, ref=b"AT", alt=b"A"), rec(pos=26, ref=b"A", alt=b"ATT"), rec(pos=27, info=b"."), rec(pos=28, info=b""),
    rec(pos=29, info=b"dp=7;Af=0.25;sb=-2;DP4=1,2,3"), rec(pos=30, info=b"DP4=1,2,3,4,5;AF=1e-3"), rec(pos=31, info=b"DP;AF;SB=x"),
    rec(pos=32, info=b"DP= 12;AF= .5;DP4=9, 8,+7,-6"), rec(pos=33, info=b"A;AF=0.5"), rec(pos=b" 34"), rec(pos=b"+35"), rec(pos=b"-3"),
    rec(b"c2", 5, extra=[b"GT", b"0/1"]), rec(b"c2", 6, extra=[b"GT"]), rec(b"c2", 7, extra=[b"GT", b"0/1", b"1/1", b""]),
    b"c2\t8\t.\tA\tG\n", b"c2\t9\t.\tA\tG\t12\n", b"c2\t10\t.\tA\tG\t12\tq9\n", b"c2\t11\t\t\t\t\t\t\n", rec(b"c1", 40), rec(b"", 41),
])
open_row("mixed_rules", MIXED)
open_row("mixed_rules_crlf", MIXED.replace(b"\n", b"\r\n"))
open_row("no_final_newline", MIXED[:-1])
open_row("double_cr", HEAD + rec(pos=3)[:-1] + b"\r\r\n" + rec(pos=4))
open_row("empty_file", b"")
open_row("one_newline", b"\n")
open_row("header_only", HEAD)
open_row("header_line_is_last_without_newline", HEAD[:-1])
open_row("header_with_format_tail", META + vm.HEADER + b"\tFORMAT\ts1\n" + rec(pos=9, extra=[b"GT", b"0/1"]))
open_row("no_chrom_line", META + rec(pos=1) + rec(pos=2))                  # the ## line is a record of one field: the records end at once
open_row("no_chrom_line_records_first", rec(pos=1) + b"#c\t2\t.\tA\tC\n" + rec(pos=3))
open_row("chrom_line_not_a_prefix_match", META + vm.HEADER[:-1] + b"\n" + rec(pos=1))
open_row("short_line_mid_file", HEAD + rec(pos=1) + rec(pos=2) + b"c1\t3\t.\tA\n" + rec(pos=4), behind=2)
open_row("empty_line_mid_file", HEAD + rec(pos=1) + b"\n" + rec(pos=4), behind=2)
open_row("second_chrom_line_is_a_record", HEAD + rec(pos=1) + vm.HEADER + b"\n" + rec(pos=2))
open_row("chrom_line_at_10000", b"##x\n" * 9999 + vm.HEADER + b"\n" + rec(pos=1), header_line=9999)
open_row("chrom_line_at_10001", b"##x\n" * 10000 + vm.HEADER + b"\n" + rec(pos=1), header_line=-1)
open_row("digits_18", HEAD + rec(pos=b"9" * 18, qual=b"9" * 9))
open_row("tabix_hash_anywhere", HEAD + rec(pos=1) + b"#late\n" + rec(pos=1, alt=b"G") + rec(b"c2", 1) + b"##x\ty\n", vm.TABIX)
open_row("tabix_end_key", HEAD + rec(pos=5, info=b"END=5") + rec(pos=6, info=b"DP=1;end=9") + rec(pos=7, info=b"END") + rec(pos=8, info=b"END=9x"),
         vm.TABIX)
open_row("tabix_end_key_no_number", HEAD + rec(pos=8, info=b"END=x9"), vm.TABIX, refused=vm.INTERVAL)      # atol gives 0

# ---- the scan's edges ------------------------------------------------------------------------------------------------------------------
for what, edge in (("chunk", CHUNK * 13), ("wave", WAVE), ("tile", TILE)):
    d = comment_to(META, edge) + vm.HEADER + b"\n" + rec(pos=1) + rec(pos=2)
    open_row("newline_ends_%s_chrom_line_starts_it" % what, d, newline=edge - 1, header=edge)
    d = comment_to(META, edge - 20) + vm.HEADER + b"\n" + rec(pos=1)
    open_row("chrom_line_straddles_%s" % what, d, header=edge - 20)
    d, nxt = records_to(HEAD, edge - 3)
    open_row("tab_ends_%s" % what, d + rec(b"c1", nxt) + rec(b"c1", nxt + 1), tab=edge - 1)
    d, nxt = records_to(HEAD, edge - 2)
    open_row("tab_starts_%s" % what, d + rec(b"c1", nxt) + rec(b"c1", nxt + 1), tab=edge)
    d, nxt = records_to(HEAD, edge + 1)
    open_row("record_ends_%s_without_newline" % what, d[:-1], size=edge)
d, nxt = records_to(HEAD, TILE)
open_row("crlf_split_across_tile", d[:-1] + b"\r\n" + rec(b"c1", nxt), cr=TILE - 1)

long_ok = rec(pos=2, info=b"DP=1;X=" + b"x" * (vm.MAX_LINE - len(rec(pos=2, info=b"DP=1;X=")) + 1))
assert len(long_ok) == vm.MAX_LINE + 1
open_row("line_of_8190", HEAD + rec(pos=1) + long_ok + rec(pos=3))
open_row("line_of_8191", HEAD + rec(pos=1) + long_ok[:-1] + b"x\n" + rec(pos=3), refused=vm.LINE_TOO_LONG)
open_row("line_of_8190_and_cr", HEAD + rec(pos=1) + long_ok[:-1] + b"\r\n" + rec(pos=3), refused=vm.LINE_TOO_LONG)

big, nxt = records_to(HEAD, (SCAN_LANES + 2) * TILE + 77)
open_row("scan_two_rounds", big + rec(b"c2", 1) + rec(b"c2", 2), size=len(big))
open_row("scan_two_rounds_tabix", big + rec(b"c2", 1) + rec(b"c2", 1), vm.TABIX)

# more lines and records than a round of the one-workgroup list scan (record list, run heads, output offsets) takes
SHORT = HEAD + b"".join(b"c%d\t%d\t.\tA\tC\n" % (i // 3000, i + 1) for i in range(LIST_ROUND + 300))
open_row("list_scan_two_rounds", SHORT, records=LIST_ROUND + 300)
open_row("list_scan_two_rounds_tabix", SHORT.replace(b"c1\t3001\t", b"#c1\t3001\t"), vm.TABIX, records=LIST_ROUND + 299)

# ---- each refusal in the first, a middle and the last tile; of two offences the earlier ------------------------------------------------
OFFENCES = {
    "too_long": (vm.STREAM, vm.LINE_TOO_LONG, long_ok[:-1] + b"x\n"),
    "nul": (vm.STREAM, vm.NUL, rec(pos=2, info=b"DP=1;X=a\0b")),
    "number_pos": (vm.STREAM, vm.NUMBER, rec(pos=b"1" * 19)),
    "number_qual": (vm.STREAM, vm.NUMBER, rec(pos=2, qual=b"1" * 10)),
    "fields": (vm.TABIX, vm.FIELDS, b"c1\t9\t.\tA\n"),
    "unsorted": (vm.TABIX, vm.UNSORTED, rec(pos=1)),
    "interval_pos": (vm.TABIX, vm.INTERVAL, rec(b"c0", 0)),
    "interval_ref": (vm.TABIX, vm.INTERVAL, rec(pos=5000000, ref=b"")),
    "interval_end": (vm.TABIX, vm.INTERVAL, rec(pos=5000000, info=b"DP=1;END=4999999")),
}
N_TILES = 6
for what, (mode, why, line) in OFFENCES.items():
    for where, at in (("first", 300), ("middle", 2 * TILE + 2000), ("last", N_TILES * TILE - 300 - len(line))):
        d, nxt = records_to(HEAD, at)
        d += line
        d, _ = records_to(d, N_TILES * TILE - 40, first=5000001)
        open_row("%s_in_%s_tile" % (what, where), d, mode, refused=why, first_tile=at // TILE, last_tile=(at + len(line) - 1) // TILE)
d, nxt = records_to(HEAD, 300)
open_row("two_offences", d + rec(pos=b"1" * 19) + rec(pos=2, info=b"\0"), refused=vm.NUMBER)
open_row("two_offences_other_order", d + rec(pos=2, info=b"\0") + rec(pos=b"1" * 19), refused=vm.NUL)
open_row("two_offences_on_one_line", d + rec(pos=b"1" * 19, info=b"\0"), refused=vm.NUL)
open_row("tabix_chrom_in_two_runs", HEAD + rec(b"c1", 5) + rec(b"c2", 1) + rec(b"c1", 9), vm.TABIX, refused=vm.UNSORTED)
open_row("stream_chrom_in_two_runs", HEAD + rec(b"c1", 5) + rec(b"c2", 1) + rec(b"c1", 3))
open_row("nul_behind_the_records", HEAD + rec(pos=1) + b"\n" + b"a\0\n", refused=vm.NUL)
open_row("number_behind_the_records", HEAD + rec(pos=1) + b"\n" + rec(pos=b"1" * 19))

# ---- vcfset ------------------------------------------------------------------------------------------------------------------------------
ONE = HEAD + b"".join([
    rec(pos=10), rec(pos=11, flt=b"PASSx"), rec(pos=12, flt=b".x"), rec(pos=13, flt=b"q20"), rec(pos=14, ref=b"AT", alt=b"A"),
    rec(pos=15, info=b"INDEL;DP=3"), rec(pos=16, info=b"DP=3;indel=1"), rec(pos=17, info=b"XINDEL"), rec(pos=b"007", qual=b"37.9"),
    rec(pos=b"12abc", qual=b".5", info=b"."), rec(pos=20, info=b""), rec(b"c2", 5, extra=[b"GT", b"0/1"]), b"c2\t6\t.\tA\tG\n",
    b"c2\t7\t.\tA\tG\t9\tq1\n", rec(b"c3", 1), rec(b"longer_chrom_name", 123456789, qual=b"."),
]).replace(b"c2\t6\t.\tA\tG\n", b"c2\t6\t.\tA\tG\r\n")
TWO = HEAD + b"".join([
    rec(pos=7, alt=b"G"), rec(pos=7), rec(pos=10), rec(pos=11, alt=b"G"), rec(pos=12, flt=b"q20"), rec(pos=13), rec(pos=14, ref=b"AT", alt=b"A", flt=b"."),
    rec(pos=15, info=b"DP=3"), rec(pos=16, info=b"INDEL"), rec(pos=16), rec(pos=20), b"#c1\t20\t.\tA\tC\n", rec(b"c2", 5), rec(b"c2", 6, alt=b"G"),
    rec(b"c2", 7, alt=b"G,T"), rec(b"longer_chrom_name", 123456789),
])
for op, opname in ((vm.INTERSECT, "intersect"), (vm.COMPLEMENT, "complement")):
    set_row(opname, ONE, TWO, op=op)
    for flag in ("only_passed", "only_pos", "only_snvs", "only_indels", "count_only"):
        set_row("%s_%s" % (opname, flag), ONE, TWO, op=op, **{flag: 1})
    set_row("%s_add_info" % opname, ONE, TWO, op=op, add=b"SOMATIC")
    set_row("%s_passed_pos_snvs" % opname, ONE, TWO, op=op, only_passed=1, only_pos=1, only_snvs=1)
TWO_PLAIN = TWO.replace(rec(b"c2", 7, alt=b"G,T"), rec(b"c2", 7, alt=b"G"))       # concat reads every file as it reads file 1
assert TWO_PLAIN != TWO and b"," not in TWO_PLAIN.replace(b"DP4=50,45,3,2", b"")
set_row("concat_one", ONE, op=vm.CONCAT)
set_row("concat_three", ONE, more=[TWO_PLAIN, META + rec(b"c9", 1) + rec(b"c9", 2), b"", HEAD], op=vm.CONCAT)
for flag in ("only_passed", "only_pos", "only_snvs", "only_indels", "count_only"):
    set_row("concat_%s" % flag, ONE, more=[TWO_PLAIN], op=vm.CONCAT, **{flag: 1})
set_row("concat_add_info", ONE, more=[TWO_PLAIN], op=vm.CONCAT, add=b"X=1;Y")
set_row("concat_no_header", rec(pos=1) + rec(pos=2), more=[HEAD + rec(pos=3)], op=vm.CONCAT)
set_row("empty_file_one", b"", TWO, op=vm.COMPLEMENT)
set_row("empty_file_two", ONE, b"", op=vm.COMPLEMENT)
# a multi-allelic ALT is longer than one byte, so it is an indel by length: --only-snvs drops it in front of the multi-allelic test, and
# --only-indels lets it through to that test, which comes in front of --only-passed
MULTI = HEAD + rec(pos=1) + rec(pos=3, alt=b"G,T", flt=b"q20") + rec(pos=4, ref=b"AT", alt=b"A,ATT") + rec(pos=5)
set_row("multiallelic_dropped_by_the_kind_filter", MULTI, TWO, op=vm.COMPLEMENT, only_snvs=1)
set_row("multiallelic_behind_the_kind_filter", MULTI, TWO, op=vm.COMPLEMENT, only_indels=1, where={"refused": vm.MULTIALLELIC, "line": 4})
set_row("multiallelic_in_front_of_only_passed", MULTI, TWO, op=vm.COMPLEMENT, only_passed=1, where={"refused": vm.MULTIALLELIC, "line": 4})
set_row("multiallelic_first_of_two", MULTI, TWO, op=vm.INTERSECT, where={"refused": vm.MULTIALLELIC, "line": 4})
set_row("multiallelic_with_only_pos", MULTI, TWO, op=vm.INTERSECT, only_pos=1)
set_row("multiallelic_in_concat_file_two", ONE, more=[MULTI], op=vm.CONCAT, where={"refused": vm.MULTIALLELIC, "line": 4, "file": 1})
set_row("pos_zero_in_file_one", HEAD + rec(pos=1) + rec(pos=0), TWO, op=vm.INTERSECT, where={"refused": vm.INTERVAL, "line": 4})
set_row("pos_zero_in_file_one_ignored", HEAD + rec(pos=1) + rec(pos=0, flt=b"q1"), TWO, op=vm.INTERSECT, only_passed=1)
set_row("pos_zero_in_concat", HEAD + rec(pos=1) + rec(pos=0) + rec(pos=b"-7"), op=vm.CONCAT)
for where, at in (("first", 300), ("middle", TILE + 2000), ("last", 3 * TILE - 300)):
    d, nxt = records_to(HEAD, at)
    d += rec(pos=nxt, alt=b"G,T")
    d, _ = records_to(d, 3 * TILE - 40, first=nxt + 1)
    set_row("multiallelic_in_%s_tile" % where, d, TWO, op=vm.COMPLEMENT, where={"refused": vm.MULTIALLELIC})

# equal-POS runs of 1, 2 and 65 records in file 2; the match first, last or absent
for n in (1, 2, 65):
    alts = [b"G" + b"T" * i for i in range(n)]
    two = HEAD + rec(pos=3) + b"".join(rec(pos=50, alt=a) for a in alts) + rec(pos=51) + rec(b"c2", 50, alt=b"Z")
    one = HEAD + rec(pos=50, alt=alts[0]) + rec(pos=50, alt=alts[-1]) + rec(pos=50, alt=b"Z") + rec(pos=2) + rec(pos=49) + rec(pos=52) + rec(b"c0", 50) + rec(b"c2", 50, alt=b"Z")
    set_row("equal_pos_run_of_%d" % n, one, two, op=vm.INTERSECT, where={"keep": [3, 3, 2, 2, 2, 2, 2, 3]})
    set_row("equal_pos_run_of_%d_complement_only_pos" % n, one, two, op=vm.COMPLEMENT, only_pos=1)
    set_row("equal_pos_run_of_%d_last_passes" % n, one, HEAD + b"".join(rec(pos=50, alt=b"G", flt=b"q1") for _ in range(n - 1)) + rec(pos=50, alt=b"G"),
            op=vm.INTERSECT, only_passed=1)

# output lines whose start, POS digits and added INFO straddle a 16-byte output chunk: every phase
PHASES = HEAD + b"".join(rec(b"c" * (1 + i % 23), 999999 + i, info=[b".", b"", b"DP=%d" % i][i % 3], qual=[b"7", b".", b"123456"][i % 3]) for i in range(120))
set_row("output_phases", PHASES, op=vm.CONCAT, add=b"ADDED_INFO_STRING=1")
set_row("output_phases_complement", PHASES, TWO, op=vm.COMPLEMENT, add=b"Z")
bigone, nxt = records_to(HEAD, 3 * TILE + 100)
set_row("more_records_than_a_scan_round", bigone, big, op=vm.INTERSECT)
set_row("more_records_than_a_scan_round_complement", big, bigone, op=vm.COMPLEMENT, where={"two_is_stream_sorted": 1})

set_row("list_scan_two_rounds_complement", SHORT, HEAD + b"".join(SHORT[len(HEAD):].splitlines(True)[::2]), op=vm.COMPLEMENT, add=b"S")

# ---- the -S mask -------------------------------------------------------------------------------------------------------------------------
MASK_VCF = HEAD + rec(pos=1) + rec(pos=2) + rec(pos=2, alt=b"G") + rec(pos=50) + rec(pos=99) + rec(pos=100) + rec(pos=101) + rec(b"c2", 7) + rec(pos=60) + rec(pos=0)
MASKS.append({"name": "mask_plain", "data": MASK_VCF, "chrom": b"c1", "ref_len": 100, "bed": None})
MASKS.append({"name": "mask_bed", "data": MASK_VCF, "chrom": b"c1", "ref_len": 100, "bed": [(0, 1), (1, 2), (40, 51), (60, 60), (99, 200)]})
MASKS.append({"name": "mask_bed_empty", "data": MASK_VCF, "chrom": b"c1", "ref_len": 100, "bed": []})
MASKS.append({"name": "mask_other_chrom", "data": MASK_VCF, "chrom": b"c2", "ref_len": 8, "bed": None})
MASKS.append({"name": "mask_absent_chrom", "data": MASK_VCF, "chrom": b"c3", "ref_len": 8, "bed": None})


def expected_open(row):
    """{"refused": (why, line)} or the model's answer in the check program's terms"""
    try:
        p = vm.parse(row["data"], row["mode"])
    except vm.Refused as e:
        return {"why": e.why, "line": e.line}
    return {"n_rec": len(p.recs), "behind": p.behind, "found": int(p.hdr_line >= 0), "header": p.header.hex(), "recs": vm.table(p),
            "runs": [[name.hex(), first] for name, first in p.runs],
            "info": [[v[0], v[1], v[2], v[3], None if v[4] is None else v[4].hex()] for v in map(vm.info_values, p.recs)]}


def expected_set(row):
    """{"open": [file, why, line]}, {"why", "file", "line"} or {"counts", "keep", "text"}; file 1 = 0, file 2 = 1, more[i] = 2 + i"""
    c = row["conf"]
    files = [row["one"], row["two"]] + row["more"]
    parsed = []
    for i, d in enumerate(files):
        if d is None:
            parsed.append(None)
            continue
        try:
            parsed.append(vm.parse(d, vm.TABIX if i == 1 else vm.STREAM))
        except vm.Refused as e:
            return {"open": [i, e.why, e.line]}
    try:
        out = vm.vcfset([parsed[0]] + parsed[2:], parsed[1], c["op"], c["only_passed"], c["only_pos"], c["only_snvs"], c["only_indels"],
                        c["count_only"], c["add"])
    except vm.Refused as e:
        return {"why": e.why, "file": e.file, "line": e.line}
    return {"counts": list(out["counts"]), "keep": out["keep"], "text": out["text"].hex()}
