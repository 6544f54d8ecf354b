"""Small inputs of lfq_bam_index_build placed on its constants: one table for the host program (tests/test_bai_edges.py) and for the
device (tests/test_gpu_bam_index.py).  A row is a body of records, its rec_off and a FABRICATED block table -- the builder takes the
tables as arguments, so nothing has to be compressed and a compressed span can be put on 65535 or 65536 at will.  What the index
of a row is comes from tests/bai_model.py; `facts`, where a row has them, are worked out by hand and hold the model to the row.
No test in here."""
import collections
import struct

import bai_model as bm
import bam_records as br

WG = br.source_constant("LFQ_BAI_THREADS", "lofreq_amd/csrc/lfq_bamidx.hip")
Row = collections.namedtuple("Row", "name body rec_off data_off comp_off file_off n_ref error facts")
W = 1 << 14
M10 = [("M", 10)]


def _row(name, recs, n_ref=2, lead=0, pieces=None, comp=None, file_off=0, error=None, facts=None, rec_off=None):
    """records one behind the other after `lead` bytes that belong to no record; pieces: the blocks' payload sizes (default: one
    block; "each": a block per record, the lead in a block of its own), comp: their compressed sizes (default 300 each)"""
    body = b"\xee" * lead + b"".join(recs)
    if rec_off is None:
        rec_off = [lead]
        for r in recs:
            rec_off.append(rec_off[-1] + len(r))
    if pieces == "each":
        pieces = ([lead] if lead else []) + [len(r) for r in recs]
    if pieces is None:
        pieces = [len(body)] if body else []
    assert sum(pieces) == len(body), (name, sum(pieces), len(body))
    comp = [300] * len(pieces) if comp is None else comp
    data_off, comp_off = [0], [0]
    for p, c in zip(pieces, comp):
        data_off.append(data_off[-1] + p)
        comp_off.append(comp_off[-1] + c)
    return Row(name, body, rec_off, data_off, comp_off, file_off, n_ref, error, facts)


def _vo(block_start, within=0):
    return (block_start << 16) | within


def _bins_are(ref, bins):
    def facts(idx):
        assert sorted(idx["refs"][ref]["bins"]) == sorted(bins), sorted(idx["refs"][ref]["bins"])
    return facts


def _chunks_are(ref, b, chunks):
    def facts(idx):
        assert idx["refs"][ref]["bins"][b] == [list(c) for c in chunks], idx["refs"][ref]["bins"].get(b)
    return facts


def _placement_rows():
    # three records in three windows, so that each is a chunk of its own and shows its u and v
    r = [bm.record(0, k * W + 5, M10, fill=k) for k in range(3)]
    n = len(r[0])
    big = bm.record(0, 5, M10, aux=b"XZZ" + b"a" * 900 + b"\0")
    rows = [
        # block 1 starts with record 1 and ends with it: v of record 0 and of record 1 are the next block's first byte
        _row("starts_and_ends_on_block_edges", r, pieces=[7 + n, n, n], comp=[50, 60, 70], lead=7, file_off=1000,
             facts=lambda idx: [_chunks_are(0, 4681 + k, [c])(idx) for k, c in enumerate((
                 (_vo(1000, 7), _vo(1050)), (_vo(1050), _vo(1110)), (_vo(1110), _vo(1180))))]),
        _row("record_across_two_blocks", [r[0], big, r[2]], pieces=[n + 100, len(big) - 100 + n], comp=[50, 60],
             facts=_chunks_are(0, 4681, [(_vo(0), _vo(50, len(big) - 100))])),
        _row("record_across_three_blocks", [r[0], big, r[2]], pieces=[n + 100, 300, len(big) - 400 + n], comp=[50, 60, 70],
             facts=_chunks_are(0, 4683, [(_vo(110, len(big) - 400), _vo(180))])),
        # an empty block between two blocks is never chosen: v of record 0 is block 2's first byte
        _row("empty_block_between", r, pieces=[n, 0, 2 * n], comp=[50, 28, 70],
             facts=_chunks_are(0, 4681, [(_vo(0), _vo(78))])),
        _row("empty_blocks_in_front_and_behind", r, pieces=[0, 3 * n, 0], comp=[28, 50, 28],
             facts=_chunks_are(0, 4683, [(_vo(28, 2 * n), _vo(106))])),
        _row("last_record_of_the_last_block", r[:1], pieces=[n], comp=[44], file_off=(1 << 40),
             facts=_chunks_are(0, 4681, [(_vo(1 << 40), _vo((1 << 40) + 44))])),
    ]
    return rows


def _boundary_rows():
    rows = []
    recs, bins = [], []
    for k, shift in enumerate((14, 17, 20, 23, 26)):
        edge = 3 << shift
        recs += [bm.record(0, edge - 10, M10, fill=k), bm.record(0, edge - 10, [("M", 11)], fill=k)]
        above = (585, 73, 9, 1, None)[k]
        bins += [4681 + ((edge - 1) >> 14), 0 if above is None else above + (edge >> (shift + 3))]
    last = (1 << 29) - 1
    recs.append(bm.record(0, last, [("M", 1)]))
    bins.append(37448)
    # (compressed blocks of 70000 bytes: every bin spans more than 65535 and none is merged away)
    rows.append(_row("ends_on_and_over_every_window_edge", recs, pieces="each", comp=[70000] * len(recs), facts=_bins_are(0, bins)))
    rows.append(_row("end_one_above_the_limit", recs + [bm.record(0, last, [("M", 2)])], error=len(recs)))
    rows.append(_row("end_above_the_limit_through_a_skip", [recs[0], bm.record(0, 1 << 20, [("M", 5), ("N", (1 << 28) - 1), ("N", (1 << 28) - 1), ("M", 5)])],
                     error=1))
    return rows


def _merge_rows():
    """a 16 kb bin with two chunks around a record of another bin, a block per record: the bin's span is the last block's end"""
    rows = []
    w = 5 * W
    child = 4681 + 5
    a, a2 = bm.record(0, w + 100, M10), bm.record(0, 6 * W - 5, [("M", 1)], fill=3)
    over = bm.record(0, 6 * W - 5, M10, fill=1)                           # across the window's edge: the 128 kb bin 585
    far = bm.record(0, 6 * W - 5, [("M", 1), ("N", 1 << 17), ("M", 1)], fill=2)   # across a 128 kb edge: bin 73, not the parent
    for span in (65535, 65536):
        comp = [100, 100, span - 200]
        merged = span < 65536
        rows.append(_row("span_%d_parent_present" % span, [a, over, a2], pieces="each", comp=comp,
                         facts=_bins_are(0, [585] if merged else [585, child])))
        rows.append(_row("span_%d_parent_absent" % span, [a, far, a2], pieces="each", comp=comp, facts=_bins_are(0, [73, child])))
    # rule 6's last step: the second chunk starts in the block where the first ends / in the one behind it
    n = len(a)
    rows.append(_row("chunk_starts_in_the_block_the_previous_ends_in", [a, far, a2], pieces=[n, len(far) + len(a2)], comp=[100, 1],
                     facts=_chunks_are(0, child, [(_vo(0), _vo(101))])))
    rows.append(_row("chunk_starts_one_block_behind", [a, far, a2], pieces="each", comp=[100, 1, 50],
                     facts=_chunks_are(0, child, [(_vo(0), _vo(100)), (_vo(101), _vo(151))])))
    return rows


def _geometry_rows():
    rows = []

    def run(n, heads, by_ref):
        recs, seg = [], 0
        for j in range(n):
            seg += j in heads
            recs.append(bm.record(seg if by_ref else 0, (0 if by_ref else seg * W) + j, M10, fill=j, flag=4 if j % 7 == 3 else 0))
        sizes, left = [], sum(len(r) for r in recs)
        while left:
            sizes.append(min(left, 1000))
            left -= sizes[-1]
        return recs, sizes

    for n in sorted({63, 64, 65, 129, WG - 1, WG, WG + 1, 2 * WG + 1}):
        heads = {h for h in (63, 64, WG, WG + 1) if h < n}
        for by_ref in (False, True):
            recs, sizes = run(n, heads, by_ref)
            want = len(heads) + 1
            rows.append(_row("%d_records_heads_at_%s_%s" % (n, "_".join(map(str, sorted(heads))) or "0", "refs" if by_ref else "bins"),
                             recs, n_ref=want + 1, pieces=sizes,
                             facts=(lambda idx, want=want, by_ref=by_ref: _count_runs(idx, want, by_ref))))
    recs, sizes = run(WG + 40, set(), False)
    rows.append(_row("one_run_longer_than_a_workgroup", recs, pieces=sizes,
                     facts=lambda idx: _chunks_are(0, 4681, [idx["refs"][0]["meta"][0]])(idx)))
    return rows


def _count_runs(idx, want, by_ref):
    with_records = [r for r in idx["refs"] if r["meta"] is not None]
    assert len(with_records) == (want if by_ref else 1)
    assert sum(len(r["bins"]) for r in with_records) == want and all(len(cs) == 1 for r in with_records for cs in r["bins"].values())


def _mix_rows():
    unm = lambda ref, pos, k=0: bm.record(ref, pos, M10, flag=4, fill=k)
    nocoor = [bm.record(-1, -1, M10, flag=4, fill=k) for k in range(3)]
    long_read = bm.record(0, 1000, [("M", 10), ("N", 100000), ("M", 10)])             # windows 0 .. 6
    shorts = [bm.record(0, k * W + 50, M10, fill=k) for k in (1, 2, 3, 8)]

    rows = [
        _row("long_read_then_short_ones_inside_its_span", [long_read] + shorts, pieces="each", comp=[70000] * 5,
             facts=lambda idx: _lin_is(idx, 0, [0] * 8 + [4])),
        _row("only_unmapped_placed_reads_in_a_reference", [bm.record(0, 5, M10), unm(1, 7), unm(1, 9, 1)], n_ref=3,
             facts=lambda idx: _assert(idx["refs"][1]["linear"] == [] and idx["refs"][1]["meta"][1] == [0, 2]
                                       and list(idx["refs"][1]["bins"]) == [4681] and idx["refs"][2]["meta"] is None)),
        _row("only_reads_without_coordinates", nocoor, facts=lambda idx: _assert(idx["n_no_coor"] == 3 and all(
            r == {"bins": {}, "linear": [], "meta": None} for r in idx["refs"]))),
        _row("one_record", [bm.record(1, 3 * W, M10)], lead=3, facts=lambda idx: _lin_is(idx, 1, [0] * 4)),
        _row("no_records", [], n_ref=3, facts=lambda idx: _assert(idx["n_no_coor"] == 0 and len(idx["refs"]) == 3)),
        _row("no_records_no_references", [], n_ref=0),
        _row("mapped_read_at_pos_minus_1", [bm.record(0, -1, [("S", 10)]), bm.record(0, -1, M10)],
             facts=lambda idx: _assert(sorted(idx["refs"][0]["bins"]) == [0, 4680] and len(idx["refs"][0]["linear"]) == 1)),
        _row("placed_then_unplaced", [bm.record(0, 5, M10), unm(1, 7)] + nocoor, pieces="each",
             facts=lambda idx: _assert(idx["n_no_coor"] == 3 and idx["refs"][1]["meta"][0][1] == _vo(600))),
    ]
    return rows


def _assert(ok):
    assert ok


def _lin_is(idx, ref, which):
    """the linear index of `ref` names, per window, the u of the record with that number among the reference's chunks' starts"""
    us = sorted(c[0] for cs in idx["refs"][ref]["bins"].values() for c in cs)
    assert idx["refs"][ref]["linear"] == [us[k] for k in which], (idx["refs"][ref]["linear"], us)


def _refusal_rows():
    good = [bm.record(0, 100 * k, M10, fill=k) for k in range(6)]
    n = len(good[0])

    def patched(rec, at, fmt, value):
        b = bytearray(rec)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)

    def swap(k, rec):
        return good[:k] + [rec] + good[k + 1:]

    off = [0]
    for r in good:
        off.append(off[-1] + len(r))
    short = good[:2] + [good[2][:20]] + good[3:]
    rows = [
        _row("block_size_is_not_the_records_length", swap(2, patched(good[2], 0, "<i", n - 3)), error=2),
        _row("record_shorter_than_its_core", short, error=2),
        _row("cigar_does_not_fit", swap(4, patched(good[4], 16, "<H", 1000)), error=4),
        _row("name_does_not_fit", swap(1, patched(good[1], 12, "<B", 255)), error=1),
        _row("ref_id_is_n_ref", swap(5, bm.record(2, 0, M10)), error=5),
        _row("ref_id_below_minus_1", swap(3, bm.record(-2, 300, M10)), error=3),
        _row("pos_below_minus_1", swap(0, bm.record(0, -2, M10)), error=0),
        _row("ref_id_goes_down", [bm.record(1, 5, M10)] + good, error=1),
        _row("placed_after_unplaced", good[:2] + [bm.record(-1, -1, M10, flag=4)] + good[2:], error=3),
        _row("pos_goes_down", swap(3, bm.record(0, 199, M10)), error=3),
        _row("two_bad_records_the_first_is_named", good[:3] + [bm.record(0, -9, M10), good[4], bm.record(7, 0, M10)], error=3),
        _row("rec_off_does_not_increase", good, rec_off=off[:3] + [off[2]] + off[4:], error=-1),
        _row("records_start_in_front_of_the_blocks", good, error=-1)._replace(data_off=[10, off[-1]]),
        _row("records_end_behind_the_blocks", good, error=-1)._replace(data_off=[0, off[-1] - 1]),
        _row("comp_off_does_not_increase", good, pieces=[n, off[-1] - n], comp=[300, 0], error=-1),
        _row("data_off_decreases", good, error=-1)._replace(data_off=[0, off[-1] + 5, off[-1]], comp_off=[0, 10, 20]),
    ]
    return rows


def _all_rows():
    rows = _placement_rows() + _boundary_rows() + _merge_rows() + _geometry_rows() + _mix_rows() + _refusal_rows()
    assert len({r.name for r in rows}) == len(rows)
    return rows


ROWS = _all_rows()


def expected(row):
    """-> the parsed index of a row by the model, or the refused record's number"""
    try:
        return bm.build(row.body, row.rec_off, row.data_off, row.comp_off, row.file_off, row.n_ref)
    except bm.BaiError as e:
        return e.record
