"""tests/bai_model.py -- the Python restatement of the .bai rules that every test of lfq_bam_index_build compares with -- held to the
.bai the reference's 2.1.4 binary wrote (tests/golden/bai_binary.json, tests/make_bai_golden.py): on the BAM the generator wrote
and on the binary's own rewrite of it (htslib's blocks).  The fixture decides: a rule of the model that disagrees with it is wrong.
Also the query the library implements: on 200 seeded regions per BAM it reaches what brute force finds.  No GPU, no library."""
import base64
import gzip
import json
import os

import numpy as np
import pytest

import bai_model as bm
import golden_util as gu

KINDS = ("python", "htslib")


class Fixture:
    def __init__(self, fx, kind):
        unz = lambda k: gzip.decompress(base64.b64decode(fx[kind][k]))
        self.bam = bm.bgzf_file(unz("payload_gz_base64"), fx[kind]["cuts"]) if kind == "python" else base64.b64decode(fx[kind]["bam_base64"])
        self.bai = unz("bai_gz_base64")
        self.want = bm.parse_bai(self.bai)
        self.got, self.data, self.rec_off, self.data_off, self.comp_off, self.refs = bm.build_from_file(self.bam)
        self.us = [bm.voffset(o, self.data_off, self.comp_off) for o in self.rec_off[:-1]]
        self.spans = [bm.record_span(self.data, o) for o in self.rec_off[:-1]]


_CACHE = {}


def load(kind):
    """the fixture's BAM `kind` with the model's index of it, computed once for every test module that asks"""
    if kind not in _CACHE:
        fx = json.load(open(os.path.join(gu.GOLDEN_DIR, "bai_binary.json")))
        _CACHE[kind] = Fixture(fx, kind)
        _CACHE[kind].idxstats = fx["idxstats"]
    return _CACHE[kind]


def regions(f, n=200, seed=5):
    """(tid, beg, end): around records of every reference -- their edges, windows and bins -- and a few that hold nothing"""
    rng = np.random.default_rng(seed)
    placed = [s for s in f.spans if s[0] >= 0]
    out = [(1, 0, 50000), (0, 0, 1 << 29), (2, 60000, 190000), (0, 99000000, 100000000), (3, 0, 1), (0, 5, 5)]
    while len(out) < n:
        ref_id, beg, end, _ = placed[int(rng.integers(len(placed)))]
        width = int(rng.choice([1, 2, 100, 1 << 14, 1 << 17, 3 << 20]))
        at = int(rng.choice([beg, end - 1, end, beg - width, beg - width + 1, (beg >> 14) << 14, ((beg >> 14) + 1) << 14]))
        at = max(at + int(rng.integers(-2, 3)), 0)
        out.append((ref_id, at, at + width))
    return out


def check_cover(f, idx_query, linear_of):
    """the contract of the query on the fixture's regions: every overlapping mapped record starts inside a chunk; the chunks are
    sorted and disjoint; none begins in front of the linear index's value"""
    for tid, beg, end in regions(f):
        chunks = idx_query(tid, beg, end)
        want = [j for j, (r, b, e, mapped) in enumerate(f.spans) if r == tid and mapped and b < end and e > beg]
        assert want == bm.overlapping(f.data, f.rec_off, tid, beg, end)
        hit = set(bm.reached(chunks, f.us))
        assert set(want) <= hit, (tid, beg, end, sorted(set(want) - hit)[:5])
        assert all(c[0] < c[1] for c in chunks) and all(a[1] < b[0] for a, b in zip(chunks, chunks[1:])), (tid, beg, end)
        lin = linear_of(tid)
        low = lin[beg >> 14] if 0 <= beg >> 14 < len(lin) else 0
        assert all(c[0] >= low for c in chunks), (tid, beg, end)


@pytest.mark.parametrize("kind", KINDS)
def test_the_model_gives_the_binarys_index(kind):
    f = load(kind)
    assert f.got["n_ref"] == f.want["n_ref"] == 5 and f.got["n_no_coor"] == f.want["n_no_coor"]
    for t, (got, want) in enumerate(zip(f.got["refs"], f.want["refs"])):
        assert got["bins"] == want["bins"], t
        assert got["linear"] == want["linear"], t
        assert got["meta"] == want["meta"], t
    assert bm.parse_bai(bm.to_bytes(f.got)) == f.want           # the model's own file reads back to the same


def test_the_two_bams_hold_the_same_records_in_other_blocks():
    a, b = load("python"), load("htslib")
    assert len(a.spans) == len(b.spans) == 979 and a.spans == b.spans
    assert a.comp_off != b.comp_off and len(a.data) < len(b.data)           # BI / BD added, htslib's block sizes
    sizes = {a.data_off[k + 1] - a.data_off[k] for k in range(len(a.data_off) - 1)}
    assert {1, 700, 65280} <= sizes                                         # blocks of mixed sizes
    inside = [k for k in a.data_off[1:-1] if k not in set(a.rec_off)]
    assert len(inside) >= 5                                                 # ... that records straddle


def test_the_golden_holds_what_it_was_made_for():
    """the generator's own assertions, on the committed file"""
    import make_bai_golden as mg
    f = load("python")
    mg.check_contents(f.bam, f.want)
    assert [tuple(r) for r in f.refs] == mg.REFS
    # the binary's idxstats: the metadata pseudo-bins' counts
    lines = [l.split("\t") for l in f.idxstats.strip().split("\n")]
    for t, (name, length, mapped, unmapped) in enumerate(lines[:5]):
        meta = f.want["refs"][t]["meta"]
        assert (name, int(length)) == mg.REFS[t] and [int(mapped), int(unmapped)] == (meta[1] if meta else [0, 0])
    assert lines[5][0] == "*" and int(lines[5][3]) == f.want["n_no_coor"]


@pytest.mark.parametrize("kind", KINDS)
def test_query_reaches_what_brute_force_finds(kind):
    f = load(kind)
    check_cover(f, lambda tid, beg, end: bm.query(f.want, tid, beg, end), lambda tid: f.want["refs"][tid]["linear"])
    assert bm.query(f.want, 1, 0, 50000) == [] and bm.query(f.want, 0, 5, 5) == [] and bm.query(f.want, 7, 0, 10) == []
    # the regions are not all trivial: most of them reach records, and a narrow one reaches far fewer than the whole file
    n_hit = sum(1 for tid, beg, end in regions(f) if bm.overlapping(f.data, f.rec_off, tid, beg, end))
    assert n_hit >= 120
    few = bm.reached(bm.query(f.want, 2, 200000, 200010), f.us)
    assert 1 <= len(few) <= 3
