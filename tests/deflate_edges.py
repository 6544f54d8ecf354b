"""Payloads for the tests of lfq_deflate.h and lfq_bgzf_deflate, each placed on a constant of the compressor or of RFC 1951.

ROWS    one Row per payload: name, payload (1 .. 65280 bytes), cap (the stream may not be larger; None: only 5 + n holds),
        btype (the block type the stream must have; None: any; a stored stream is 5 + n bytes exactly)
The caps are derived, not tuned: 1 bit per literal is the floor of any Huffman-only coder, a fixed-code literal costs 8 - 9 bits.
    const      one byte repeated: Huffman-only needs 8160 bytes; 2048 proves matches of 258 at distance 1 across the whole block
    period300  300 random bytes repeated: 4096 proves matches beyond one 64-position step
    sym4       uniform over 4 byte values: fixed codes need 0.42 n even with zlib's matcher; 0.35 n proves dynamic codes
    qual41     uniform over 33 .. 73: fixed codes 0.97 n, Huffman-only 0.68 n; 0.72 n proves the same on a wide alphabet
    rand256    uniform over 256 values: the stored fall-back, 5 + n bytes exactly
tests/test_deflate_edges.py holds the table to zlib (level 6 stays within every cap).  No test in here."""
import collections

import numpy as np

import bam_records as br
import bgzf_edges as be

Row = collections.namedtuple("Row", "name payload cap btype")
STEP = br.source_constant("LFQ_DEF_STEP", "lofreq_amd/csrc/lfq_deflate.h")
MAX_IN = br.source_constant("LFQ_DEF_MAX_IN", "lofreq_amd/csrc/lfq_deflate.h")
N = 65280


def _rand(rng, n, lo=0, hi=256):
    return bytes(rng.integers(lo, hi, int(n)).astype(np.uint8))


def _rows():
    assert MAX_IN == N
    R = []
    add = lambda name, payload, cap=None, btype=None: R.append(Row(name, bytes(payload), cap, btype))
    # ---- sizes: the smallest, the step's edges, the largest
    for n in (1, 2, 3, 4, STEP - 1, STEP, STEP + 1, 2 * STEP - 1, 2 * STEP, 2 * STEP + 1, N - 1, N):
        add("size_%d" % n, be._payload(n, 10 + n % 7))
    # ---- match lengths: a segment that stands twice, with different bytes around both copies
    for k in (2, 3, 257, 258, 259, 600):
        rng = np.random.default_rng(100 + k)
        seg = _rand(rng, k, 0, 200)
        add("match_len_%d" % k, _rand(rng, 2 * STEP, 0, 200) + b"\xc8" + seg + b"\xc9" + _rand(rng, STEP + 6, 0, 200) + b"\xca" + seg
            + b"\xcb" + _rand(rng, 9, 0, 200))
    # ---- distances
    add("distance_1", b"front" + b"z" * 300 + b"back")
    for d in (STEP - 1, STEP, STEP + 1, 32767, 32768):
        rng = np.random.default_rng(200 + d)
        word = _rand(rng, 40, 1, 256)       # (one byte value in between: the word's place in the hash table is still its own)
        add("distance_%d" % d, word + b"\0" * (d - 40) + word + _rand(rng, 11, 1, 256))
    rng = np.random.default_rng(32769)
    far = _rand(rng, 32769)
    # the only match is out of reach: with it the dynamic block would win (about 32.9 kB), without it the stored one does
    add("distance_32769", far + far[:300], None, 0)
    # ---- alphabets
    add("one_byte_value", b"\x07" * 1000)
    add("two_byte_values", _rand(np.random.default_rng(5), 3000, 65, 67))
    add("all_256_once", bytes(np.random.default_rng(6).permutation(256).astype(np.uint8)))    # no match: no distance symbol
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    deep = np.repeat(np.arange(22, dtype=np.uint8) + 40, fib)       # Huffman lengths up to 21 before they are limited
    np.random.default_rng(7).shuffle(deep)
    assert len(deep) == sum(fib) <= N
    add("fibonacci_22_symbols", deep.tobytes())
    rng = np.random.default_rng(8)
    pool = _rand(rng, 258)
    every = bytes(range(256)) + pool
    for length in be.LBASE + [4, 12, 30, 100, 200, 257]:           # a match of every length class offered
        every += _rand(rng, STEP + 7) + pool[:length]
    add("every_length_class", every)
    # ---- BAM records with qualities
    add("bam_records", b"".join(be.bam_record(br.mk(100 + i % 3, seed=i, pos0=1000 + 7 * i, name="read%d" % i)) for i in range(150)))
    # ---- the rows with a cap (numpy's default_rng(1), n = 65280)
    rng = np.random.default_rng(1)
    add("const", b"Q" * N, 2048)
    add("period300", (_rand(rng, 300) * (N // 300 + 1))[:N], 4096)
    add("sym4", bytes(np.array([3, 17, 90, 200], np.uint8)[rng.integers(0, 4, N)]), int(0.35 * N))
    add("qual41", _rand(rng, N, 33, 74), int(0.72 * N))
    add("rand256", _rand(rng, N), None, 0)                        # (zlib splits it into two stored blocks: 65290)
    assert all(0 < len(r.payload) <= N for r in R) and len({r.name for r in R}) == len(R)
    return R


ROWS = _rows()
