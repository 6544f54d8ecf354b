/*
 * lfq_inflate.h -- what a raw deflate stream (RFC 1951) means, for the host and for the device: the bit reader, the stored-block
 * check, the fixed tables, the construction of the dynamic tables and the symbol loop.  lfq_bgzf.hip runs it with one wavefront
 * per BGZF block (SAM specification section 4.1), lfq_inflate_check.cpp with the host compiler as a stand-alone program
 * (tests/test_bgzf_edges.py).  Both instantiate lfq_inflate() with an `Io` that says how bytes are fetched and stored and
 * nothing else: what is decoded, and what is refused, is decided here.
 *
 * Io (lfq_bgzf.hip: LfqInfDevIo, lfq_inflate_check.cpp: HostIo) provides
 *     uint32_t in8(int64_t p), in32(int64_t p)   the input byte at p / the four bytes from p on, little-endian.  Only called
 *                                                for in_beg <= p and p + 1 (p + 4) <= in_end
 *     void lit(uint32_t at, uint32_t v)          output byte `at` is v
 *     void match(uint32_t at, uint32_t dist, uint32_t len)   output bytes [at, at + len) repeat those from at - dist on, as a
 *                                                byte-by-byte copy does (dist < len: the copy reads what it wrote)
 *     void stored(uint32_t at, int64_t p, uint32_t len)      output bytes [at, at + len) are input bytes [p, p + len)
 *     int lane(), lanes()                        the table fills are cut over lanes() workers; lane() is this one's number
 *     void sync()                                what one worker wrote to the tables is visible to the others
 * Output positions count from the block's first byte.  Every call is made with positions already checked: at + len <= out_end,
 * dist <= at, p + len <= in_end.
 *
 * Termination on any input: every trip of a loop below consumes at least one input bit or produces at least one output byte or
 * one code length, and the position is compared with its limit (in_end, out_end, the number of lengths) before use.
 *
 * Status of a block, 0 or the first thing found wrong:
 */
#ifndef LFQ_INFLATE_H
#define LFQ_INFLATE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define LFQ_INF_FN __host__ __device__ static inline
#else
#define LFQ_INF_FN static inline
#endif

#define LFQ_INF_OK 0
#define LFQ_INF_MALFORMED 1     /* deflate data no decoder accepts: block type 3, LEN != ~NLEN, a bad code-length set, a code that is
                                   not assigned, length symbol 286 / 287, distance symbol 30 / 31, no end-of-block code */
#define LFQ_INF_TRUNCATED 2     /* the input ends inside a symbol, a block header or a stored block */
#define LFQ_INF_OVERRUN 3       /* a symbol would write past ISIZE */
#define LFQ_INF_DISTANCE 4      /* a match reaches before the first byte of the block's own output */
#define LFQ_INF_SIZE 5          /* the stream ends with fewer than ISIZE bytes written */
#define LFQ_INF_CRC 6           /* the CRC-32 of the output is not the trailer's */

#define LFQ_INF_MAXBITS 15
#define LFQ_INF_FAST_BITS 10    /* codes of up to this many bits are looked up, longer ones walked */
#define LFQ_INF_CLEN_FAST_BITS 7 /* ... of the code-length code: all of them */
#define LFQ_INF_MAX_OUT 65536   /* a BGZF block inflates to at most this */

/* one canonical Huffman code: per length L the first code, where its symbols start in sym[], and limit[L] = one past the last code
 * of length <= L, shifted to 15 bits.  fast[bits] caches lfq_inf_walk() for codes of up to fast_bits bits. */
struct LfqInfCode {
    uint16_t limit[LFQ_INF_MAXBITS + 1];
    uint16_t first[LFQ_INF_MAXBITS + 1];
    uint16_t offs[LFQ_INF_MAXBITS + 1];
    uint16_t sym[288];
    uint16_t fast[1 << LFQ_INF_FAST_BITS];      /* (symbol << 4) | length; 0 = walk.  The first 2^fast_bits entries are in use */
};

/* the tables of one block in flight (the device keeps them in LDS) */
struct LfqInfTables {
    LfqInfCode lit, dist;               /* (the code-length code lives in `dist` until the distance code is built) */
    uint8_t lens[288 + 32];             /* code lengths: literal/length symbols, then distance symbols */
    uint16_t lbase[32], dbase[32];      /* length symbols 257 + i, distance symbols i: base value, extra bits */
    uint8_t lext[32], dext[32];
};

/* RFC 1951 section 3.2.5 */
LFQ_INF_FN void lfq_inf_fill_bases(LfqInfTables *T, int lane, int lanes)
{
    const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
                                227, 258};
    const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                                4097, 6145, 8193, 12289, 16385, 24577};
    const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    for (int i = lane; i < 32; i += lanes) {
        T->lbase[i] = i < 29 ? lbase[i] : 0;
        T->lext[i] = i < 29 ? lext[i] : 0;
        T->dbase[i] = i < 30 ? dbase[i] : 0;
        T->dext[i] = i < 30 ? dext[i] : 0;
    }
}

LFQ_INF_FN uint32_t lfq_inf_rev15(uint32_t v)   /* the low 15 bits, first bit read -> most significant */
{
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
    v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
    return v >> 1;
}

/* the symbol whose code starts the 15 bits `bits` (first bit read = bit 0): (symbol << 4) | length, or 0 = no code of this set */
LFQ_INF_FN uint32_t lfq_inf_walk(const LfqInfCode *C, uint32_t bits)
{
    const uint32_t v = lfq_inf_rev15(bits & 0x7fffu);
    for (int L = 1; L <= LFQ_INF_MAXBITS; L++) {
        if (v < C->limit[L]) {
            return ((uint32_t)C->sym[C->offs[L] + ((v >> (LFQ_INF_MAXBITS - L)) - C->first[L])] << 4) | (uint32_t)L;
        }
    }
    return 0;
}

LFQ_INF_FN uint32_t lfq_inf_lookup(const LfqInfCode *C, uint32_t bits, int fast_bits)    /* fast_bits: what the code was built with */
{
    const uint32_t e = C->fast[bits & ((1u << fast_bits) - 1u)];
    return e ? e : lfq_inf_walk(C, bits);
}

/* The code of n lengths (0 = symbol not used).  Refused as zlib refuses them: an over-subscribed set, and an incomplete one unless
 * it is a single code of one bit (allow_single: the literal/length and the distance code, never the code-length code).  A set
 * without any code is built empty -- every lookup fails -- when allow_single. */
template <class Io>
LFQ_INF_FN int lfq_inf_build(LfqInfCode *C, const uint8_t *lens, int n, int fast_bits, bool allow_single, Io &io)
{
    int count[LFQ_INF_MAXBITS + 1];
    for (int L = 0; L <= LFQ_INF_MAXBITS; L++) {
        count[L] = 0;
    }
    for (int i = 0; i < n; i++) {
        count[lens[i] & 15]++;
    }
    int left = 1, used = 0, maxl = 0;
    for (int L = 1; L <= LFQ_INF_MAXBITS; L++) {
        left = 2 * left - count[L];
        if (left < 0) {
            return LFQ_INF_MALFORMED;           /* over-subscribed */
        }
        used += count[L];
        if (count[L]) {
            maxl = L;
        }
    }
    if (used == 0 ? !allow_single : (left > 0 && !(allow_single && maxl == 1))) {
        return LFQ_INF_MALFORMED;               /* incomplete */
    }
    io.sync();                                  /* (nobody still reads the code this one replaces) */
    if (io.lane() == 0) {
        uint32_t code = 0, at = 0;
        int fill[LFQ_INF_MAXBITS + 1];
        C->limit[0] = C->first[0] = C->offs[0] = 0;
        for (int L = 1; L <= LFQ_INF_MAXBITS; L++) {
            code = (code + (uint32_t)count[L - 1] * (L > 1)) << 1;
            C->first[L] = (uint16_t)code;
            C->offs[L] = (uint16_t)at;
            fill[L] = (int)at;
            at += (uint32_t)count[L];
            C->limit[L] = (uint16_t)((code + (uint32_t)count[L]) << (LFQ_INF_MAXBITS - L));
        }
        for (int i = 0; i < n; i++) {           /* symbols in order within a length */
            const int L = lens[i] & 15;
            if (L) {
                C->sym[fill[L]++] = (uint16_t)i;
            }
        }
    }
    io.sync();
    for (uint32_t i = (uint32_t)io.lane(); i < (1u << fast_bits); i += (uint32_t)io.lanes()) {
        const uint32_t e = lfq_inf_walk(C, i);
        C->fast[i] = (uint16_t)((e & 15u) && (int)(e & 15u) <= fast_bits ? e : 0u);
    }
    io.sync();
    return LFQ_INF_OK;
}

/* the bit reader: bits [0, n) of `bb` are the next n unread bits of the input, `pos` the first byte not yet in bb */
struct LfqInfBits {
    uint64_t bb;
    int32_t n;
    int64_t pos, end;
};

/* at least 32 bits in bb unless the input has fewer left; the bits behind the input's end read as 0 and are never consumed:
 * every consumer compares its need with n first */
template <class Io>
LFQ_INF_FN void lfq_inf_refill(LfqInfBits *B, Io &io)
{
    if (B->n <= 32) {
        if (B->pos + 4 <= B->end) {
            B->bb |= (uint64_t)io.in32(B->pos) << B->n;
            B->pos += 4;
            B->n += 32;
        } else {
            while (B->n <= 56 && B->pos < B->end) {
                B->bb |= (uint64_t)io.in8(B->pos) << B->n;
                B->pos += 1;
                B->n += 8;
            }
        }
    }
}

LFQ_INF_FN uint32_t lfq_inf_take(LfqInfBits *B, int k)   /* k <= n, k <= 16 */
{
    const uint32_t v = (uint32_t)B->bb & ((1u << k) - 1u);
    B->bb >>= k;
    B->n -= k;
    return v;
}

/* the code lengths of a dynamic block (RFC 1951 section 3.2.7) into T->lens, and both codes built */
template <class Io>
LFQ_INF_FN int lfq_inf_dynamic(LfqInfTables *T, LfqInfBits *B, Io &io)
{
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    lfq_inf_refill(B, io);
    if (B->n < 14) {
        return LFQ_INF_TRUNCATED;
    }
    const int nlen = (int)lfq_inf_take(B, 5) + 257, ndist = (int)lfq_inf_take(B, 5) + 1, ncode = (int)lfq_inf_take(B, 4) + 4;
    if (nlen > 286 || ndist > 30) {
        return LFQ_INF_MALFORMED;
    }
    uint8_t cl[19];
    for (int i = 0; i < 19; i++) {
        cl[i] = 0;
    }
    for (int i = 0; i < ncode; i++) {
        lfq_inf_refill(B, io);
        if (B->n < 3) {
            return LFQ_INF_TRUNCATED;
        }
        cl[order[i]] = (uint8_t)lfq_inf_take(B, 3);
    }
    int rc = lfq_inf_build(&T->dist, cl, 19, LFQ_INF_CLEN_FAST_BITS, false, io);
    if (rc != LFQ_INF_OK) {
        return rc;
    }
    /* one run of nlen + ndist lengths: a repeat may run from the literal/length lengths on into the distance lengths */
    const int total = nlen + ndist;
    int have = 0;
    while (have < total) {
        lfq_inf_refill(B, io);
        const uint32_t e = lfq_inf_lookup(&T->dist, (uint32_t)B->bb, LFQ_INF_CLEN_FAST_BITS);
        const int L = (int)(e & 15u), s = (int)(e >> 4);
        if (!L) {
            return B->n < 7 ? LFQ_INF_TRUNCATED : LFQ_INF_MALFORMED;
        }
        if (L > B->n) {
            return LFQ_INF_TRUNCATED;
        }
        (void)lfq_inf_take(B, L);
        if (s < 16) {
            if (io.lane() == 0) {
                T->lens[have] = (uint8_t)s;
            }
            have++;
            continue;
        }
        const int xb = s == 16 ? 2 : s == 17 ? 3 : 7, base = s == 18 ? 11 : 3;
        if (xb > B->n) {
            return LFQ_INF_TRUNCATED;
        }
        const int rep = base + (int)lfq_inf_take(B, xb);
        if (s == 16 && have == 0) {
            return LFQ_INF_MALFORMED;           /* nothing to repeat */
        }
        if (rep > total - have) {
            return LFQ_INF_MALFORMED;
        }
        io.sync();                              /* (lens[have - 1] may be another worker's store) */
        const uint8_t v = s == 16 ? T->lens[have - 1] : (uint8_t)0;
        if (io.lane() == 0) {
            for (int k = 0; k < rep; k++) {
                T->lens[have + k] = v;
            }
        }
        io.sync();
        have += rep;
    }
    io.sync();
    if (T->lens[256] == 0) {
        return LFQ_INF_MALFORMED;               /* no end-of-block code */
    }
    /* the distance lengths move behind 288 so that both sets stay where the fixed block has them; the code-length code in
     * T->dist is done with */
    uint8_t dl[32];
    for (int i = 0; i < 32; i++) {
        dl[i] = i < ndist ? T->lens[nlen + i] : (uint8_t)0;
    }
    io.sync();
    if (io.lane() == 0) {
        for (int i = nlen; i < 288; i++) {
            T->lens[i] = 0;
        }
        for (int i = 0; i < 32; i++) {
            T->lens[288 + i] = dl[i];
        }
    }
    io.sync();
    rc = lfq_inf_build(&T->lit, T->lens, 288, LFQ_INF_FAST_BITS, true, io);
    if (rc != LFQ_INF_OK) {
        return rc;
    }
    return lfq_inf_build(&T->dist, T->lens + 288, 32, LFQ_INF_FAST_BITS, true, io);
}

/* the fixed codes (RFC 1951 section 3.2.6): 288 literal/length and 32 distance symbols; 286, 287, 30 and 31 have codes and are
 * refused where they are used */
template <class Io>
LFQ_INF_FN int lfq_inf_fixed(LfqInfTables *T, Io &io)
{
    io.sync();
    for (int i = io.lane(); i < 320; i += io.lanes()) {
        T->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
    }
    io.sync();
    const int rc = lfq_inf_build(&T->lit, T->lens, 288, LFQ_INF_FAST_BITS, true, io);
    if (rc != LFQ_INF_OK) {
        return rc;
    }
    return lfq_inf_build(&T->dist, T->lens + 288, 32, LFQ_INF_FAST_BITS, true, io);
}

/* the symbols of one compressed block, until its end-of-block code */
template <class Io>
LFQ_INF_FN int lfq_inf_symbols(const LfqInfTables *T, LfqInfBits *B, uint32_t *out_io, uint32_t out_end, Io &io)
{
    uint32_t out = *out_io;
    for (;;) {
        lfq_inf_refill(B, io);
        uint32_t e = lfq_inf_lookup(&T->lit, (uint32_t)B->bb, LFQ_INF_FAST_BITS);
        int L = (int)(e & 15u);
        uint32_t s = e >> 4;
        if (!L) {
            *out_io = out;
            return B->n < LFQ_INF_MAXBITS ? LFQ_INF_TRUNCATED : LFQ_INF_MALFORMED;
        }
        if (L > B->n) {
            *out_io = out;
            return LFQ_INF_TRUNCATED;
        }
        (void)lfq_inf_take(B, L);
        if (s < 256) {
            if (out >= out_end) {
                *out_io = out;
                return LFQ_INF_OVERRUN;
            }
            io.lit(out, s);
            out++;
            continue;
        }
        *out_io = out;
        if (s == 256) {
            return LFQ_INF_OK;
        }
        s -= 257;
        if (s >= 29) {
            return LFQ_INF_MALFORMED;           /* 286, 287 */
        }
        int xb = T->lext[s];
        if (xb > B->n) {
            return LFQ_INF_TRUNCATED;
        }
        const uint32_t len = T->lbase[s] + lfq_inf_take(B, xb);
        lfq_inf_refill(B, io);
        e = lfq_inf_lookup(&T->dist, (uint32_t)B->bb, LFQ_INF_FAST_BITS);
        L = (int)(e & 15u);
        s = e >> 4;
        if (!L) {
            return B->n < LFQ_INF_MAXBITS ? LFQ_INF_TRUNCATED : LFQ_INF_MALFORMED;
        }
        if (L > B->n) {
            return LFQ_INF_TRUNCATED;
        }
        (void)lfq_inf_take(B, L);
        if (s >= 30) {
            return LFQ_INF_MALFORMED;           /* 30, 31 */
        }
        xb = T->dext[s];
        if (xb > B->n) {
            return LFQ_INF_TRUNCATED;
        }
        const uint32_t dist = T->dbase[s] + lfq_inf_take(B, xb);
        if (dist > out) {
            return LFQ_INF_DISTANCE;
        }
        if (len > out_end - out) {
            return LFQ_INF_OVERRUN;
        }
        io.match(out, dist, len);
        out += len;
    }
}

/* One deflate stream: input bytes [in_beg, in_end), output bytes [0, out_end).  -> status; *n_out = the bytes written.  Bytes
 * behind the final block's end are ignored.  T->lbase .. dext are filled here. */
template <class Io>
LFQ_INF_FN int lfq_inflate(LfqInfTables *T, int64_t in_beg, int64_t in_end, uint32_t out_end, uint32_t *n_out, Io &io)
{
    LfqInfBits B;
    B.bb = 0;
    B.n = 0;
    B.pos = in_beg;
    B.end = in_end;
    uint32_t out = 0;
    *n_out = 0;
    lfq_inf_fill_bases(T, io.lane(), io.lanes());
    io.sync();
    for (;;) {                                  /* one deflate block a trip: at least its three header bits are consumed */
        lfq_inf_refill(&B, io);
        if (B.n < 3) {
            *n_out = out;
            return LFQ_INF_TRUNCATED;
        }
        const uint32_t last = lfq_inf_take(&B, 1), type = lfq_inf_take(&B, 2);
        int rc = LFQ_INF_OK;
        if (type == 0) {
            (void)lfq_inf_take(&B, B.n & 7);    /* to the byte boundary; then LEN, NLEN */
            lfq_inf_refill(&B, io);
            if (B.n < 32) {
                rc = LFQ_INF_TRUNCATED;
            } else {
                const uint32_t len = lfq_inf_take(&B, 16), nlen = lfq_inf_take(&B, 16);
                B.pos -= B.n >> 3;              /* the whole bytes still in bb are the stored block's */
                B.bb = 0;
                B.n = 0;
                if (len != (nlen ^ 0xffffu)) {
                    rc = LFQ_INF_MALFORMED;
                } else if ((int64_t)len > B.end - B.pos) {
                    rc = LFQ_INF_TRUNCATED;
                } else if (len > out_end - out) {
                    rc = LFQ_INF_OVERRUN;
                } else {
                    if (len) {
                        io.stored(out, B.pos, len);
                    }
                    B.pos += len;
                    out += len;
                }
            }
        } else if (type == 3) {
            rc = LFQ_INF_MALFORMED;
        } else {
            rc = type == 1 ? lfq_inf_fixed(T, io) : lfq_inf_dynamic(T, &B, io);
            if (rc == LFQ_INF_OK) {
                rc = lfq_inf_symbols(T, &B, &out, out_end, io);
            }
        }
        *n_out = out;
        if (rc != LFQ_INF_OK) {
            return rc;
        }
        if (last) {
            return out == out_end ? LFQ_INF_OK : LFQ_INF_SIZE;
        }
    }
}

/* ---- CRC-32 (gzip: polynomial 0xEDB88320, bits reflected) ----------------------------------------------------------------------
 * A slice's CRC is computed from its bytes with the byte table; slices are combined by multiplication by x^(8 len) modulo the
 * polynomial: crc(A | B) = crc(A) * x^(8 |B|) + crc(B), so that the CRC of a block is the sum over its slices of
 * crc(slice) * x^(8 * bytes behind the slice). */
#define LFQ_CRC_POLY 0xedb88320u
#define LFQ_CRC_SLICES 64       /* the device: one per lane */

/* the bytes of a slice when n bytes are cut into LFQ_CRC_SLICES: whole dwords, the last slices short or empty */
LFQ_INF_FN uint32_t lfq_crc_slice_bytes(uint32_t n)
{
    return ((n + LFQ_CRC_SLICES - 1) / LFQ_CRC_SLICES + 3u) & ~3u;
}

LFQ_INF_FN uint32_t lfq_crc_table_entry(uint32_t i)
{
    uint32_t c = i;
    for (int k = 0; k < 8; k++) {
        c = (c & 1u) ? (c >> 1) ^ LFQ_CRC_POLY : c >> 1;
    }
    return c;
}

/* a * b modulo the polynomial; bit 31 is x^0 */
LFQ_INF_FN uint32_t lfq_crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int k = 0; k < 32; k++) {
        if (a & (0x80000000u >> k)) {
            p ^= b;
        }
        b = (b & 1u) ? (b >> 1) ^ LFQ_CRC_POLY : b >> 1;
    }
    return p;
}

/* x^(8 n) modulo the polynomial, n < 2^28 */
LFQ_INF_FN uint32_t lfq_crc_x8n(uint32_t n)
{
    uint32_t r = 0x80000000u, sq = 0x00800000u;         /* x^0, x^8 */
    for (int k = 0; k < 28; k++) {
        if ((n >> k) & 1u) {
            r = lfq_crc_mul(r, sq);
        }
        sq = lfq_crc_mul(sq, sq);
    }
    return r;
}

#endif
