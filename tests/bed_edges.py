"""One table of (BED text, name, queries) rows on the edges of lofreq_amd/csrc/lfq_bed.h: the binary search over the sorted
begins, the running maximum of the ends, the parser's number rules.  tests/test_bed_edges.py runs the header's stand-alone program
over it, tests/test_abi_bed.py the library's host functions, tests/test_gpu_bed.py the read kernel (the queries as reads); the
expected answers are tests/bed_model.py's.  A query is a half-open [beg, end) of at most 200 bases."""
import collections

import numpy as np

import bed_model as bm

INT32_MAX = bm.INT32_MAX
Row = collections.namedtuple("Row", "name text contig queries")


def _text(contig, iv):
    return "".join("%s\t%d\t%d\n" % (contig, b, e) for b, e in iv)


def _around(iv, rng, n_random=40, span=30000):
    """queries on every edge of a few intervals, and random ones"""
    q = []
    for b, e in iv[:3] + iv[-3:] + [iv[len(iv) // 2]] if iv else []:
        for x in (b, e):
            for lo in (x - 2, x - 1, x, x + 1):
                if lo >= 0:
                    q += [(lo, lo + 1), (lo, lo + 2)]
    for _ in range(n_random):
        lo = int(rng.integers(0, span))
        q.append((lo, lo + int(rng.integers(1, 120))))
    return q


def _table(n, seed):
    """n intervals of mixed length, some overlapping, some zero-length, begins not unique"""
    rng = np.random.default_rng(seed)
    beg = np.sort(rng.integers(50, 20000, n))
    iv = [(int(b), int(b) + int(rng.choice([0, 1, 2, 15, 40, 400]))) for b in beg]
    rng.shuffle(iv)                                         # the text is not sorted; the table is
    return [tuple(x) for x in iv], rng


def rows():
    out = []
    for n in (0, 1, 2, 3, 63, 64, 65, 1000):
        iv, rng = _table(n, 100 + n)
        text = _text("c1", iv) if n else "# nothing\n"
        out.append(Row("table_of_%d" % n, text, "c1", _around(sorted(iv), rng) + [(0, 1), (0, 50), (25000, 25100)]))
    out.append(Row("touching_is_no_overlap", "c1\t100\t200\n", "c1",
                   [(50, 100), (99, 100), (99, 101), (100, 101), (199, 200), (199, 201), (200, 201), (200, 260), (150, 151)]))
    # a zero-length interval [x, x) against a read [pos, endpos) = [100, 150): at pos, pos + 1, endpos - 1, endpos
    for x in (100, 101, 149, 150):
        out.append(Row("zero_length_at_%d" % x, "c1\t%d\t%d\n" % (x, x), "c1",
                       [(100, 150), (x, x + 1), (x - 1, x), (x - 1, x + 1), (x - 1, x + 2)]))
    # what the running maximum is for: a long early interval reaches a query far behind many short later ones
    short = [(1000 + 10 * i, 1000 + 10 * i + 3) for i in range(300)]
    out.append(Row("long_early_interval", _text("c1", [(10, 3900)] + short), "c1",
                   [(3885, 3888), (3896, 3899), (3899, 3900), (3903, 3908), (3995, 3999), (3990, 3991), (5, 10), (9, 11), (4000, 4100)]))
    out.append(Row("long_early_interval_ends_first", _text("c1", [(10, 1500)] + short), "c1",
                   [(1495, 1499), (1499, 1500), (1500, 1501), (1503, 1510), (1504, 1509), (3993, 3994), (3995, 3999)]))
    out.append(Row("in_front_and_behind", "c1\t500\t600\nc1\t700\t800\n", "c1",
                   [(0, 1), (0, 500), (400, 500), (499, 500), (499, 501), (600, 700), (650, 660), (800, 801), (800, 900), (799, 800),
                    (100000, 100100)]))
    out.append(Row("other_names_do_not_count", "c2\t0\t1000\nc1\t500\t600\nc3\t0\t1000\n", "c1", [(0, 100), (550, 560), (600, 601)]))
    out.append(Row("name_not_in_the_bed", "c2\t0\t1000\n", "c1", [(0, 100), (550, 560)]))
    out.append(Row("at_int32_max", "c1\t%d\t%d\nc1\t%d\n" % (INT32_MAX - 10, INT32_MAX, INT32_MAX - 100), "c1",
                   [(INT32_MAX - 1, INT32_MAX), (INT32_MAX - 11, INT32_MAX - 10), (INT32_MAX - 12, INT32_MAX - 9),
                    (INT32_MAX - 101, INT32_MAX - 100), (INT32_MAX - 100, INT32_MAX - 99), (INT32_MAX - 50, INT32_MAX - 40)]))
    out.append(Row("list_format_and_signs", "c1 +100 +110\nc1 205 rs7\nc1 300.5 400\nc1\t7\t7\n", "c1",
                   [(99, 100), (100, 101), (109, 110), (110, 111), (203, 204), (204, 205), (205, 206), (299, 300), (300, 301), (6, 8)]))
    return out


# texts the parser refuses -> the 1-based line
REFUSED = [
    ("no_number", "c1\t1\t2\nc1\n", 2),
    ("letters", "c1\tabc\t5\n", 1),
    ("end_below_beg", "c1\t9\t8\n", 1),
    ("list_zero", "c1 0\n", 1),
    ("negative_beg", "c1 -5 7\n", 1),
    ("negative_end", "c1 5 -7\n", 1),
    ("above_int32_max", "c1\t5\t%d\n" % (INT32_MAX + 1), 1),
    ("list_above_int32_max", "c1 %d\n" % (INT32_MAX + 1), 1),
    ("far_above", "c1\t1\t99999999999999999999999\n", 1),
    ("after_skipped_lines", "track x\n#\n  \nbrowser 9 1\nc1 x\n", 5),
]
ACCEPTED_ODD = [
    ("int32_max_itself", "c1\t0\t%d\n" % INT32_MAX, {"c1": [(0, INT32_MAX)]}),
    ("list_int32_max", "c1 %d\n" % INT32_MAX, {"c1": [(INT32_MAX - 1, INT32_MAX)]}),
    ("track_and_browser_with_bad_numbers", "track 9 1\nbrowser\nc1\t1\t2\n", {"c1": [(1, 2)]}),
    ("empty_text", "", {}),
    ("only_a_newline", "\n", {}),
    ("nul_ends_the_line", "c1\t1\t2\0 junk\nc1\t5\t6\n", {"c1": [(1, 2), (5, 6)]}),
    ("minus_zero", "c1 -0 4\n", {"c1": [(0, 4)]}),
]

ROWS = rows()


def expected(row):
    """-> the model's answers to the row's queries"""
    iv = bm.parse(row.text).get(row.contig, [])
    return [1 if bm.overlap(iv, b, e) else 0 for b, e in row.queries]
