/*
 * lfq_deflate.h -- one payload of 0 < n <= 65280 bytes written as one raw deflate stream (RFC 1951) that is a single block with
 * BFINAL = 1, for the host and for the device: the sibling of lfq_inflate.h.  lfq_bgzf_deflate.hip runs it with one wavefront per
 * BGZF block, lfq_deflate_check.cpp with the host compiler as a stand-alone program (tests/test_deflate_edges.py).  Both
 * instantiate lfq_deflate() with an `Io`; which bytes the stream holds is decided here and is a function of the payload alone.
 *
 * Io (lfq_bgzf_deflate.hip: LfqDefDevIo, lfq_deflate_check.cpp: HostIo) provides
 *     int lane(), lanes()                      loops over positions and table entries are cut over lanes() workers
 *     void sync()                              what one worker wrote to the state is visible to the others
 *     bool any(bool v)                         v of any worker, the same answer for all of them
 *     uint32_t ld8(uint32_t p), ld32(uint32_t p)   payload byte p / the four bytes from p on, little-endian; p + 1 (p + 4) <= n
 *     void out32(uint32_t w, uint32_t v)       dword w of the stream is v; w < (5 + n + 3) / 4, each dword written once
 *     void add32(uint32_t *p, uint32_t v), or32(uint32_t *p, uint32_t v)   *p += v, *p |= v on a word of the state that several
 *                                              workers may update in one step (commutative, so the order does not matter)
 *
 * The matcher, in terms of positions.  The payload is walked in steps of LFQ_DEF_STEP positions.  A table maps the hash of three
 * bytes to the LAST position in front of the current step whose three bytes have that hash.  The candidate of position p is that
 * position for the bytes at p -- so it never lies in p's own step --, refused when it is more than 32768 back; its length is the
 * common prefix, at most 258 and at most n - p.  A candidate is a match when its length is at least 3 and its estimated cost,
 * LFQ_DEF_SYM_COST bits for the two symbols plus the extra bits of length and distance, is below length x the payload's average
 * literal cost (the entropy of its byte histogram in 1/16 bit, at least one bit: what a Huffman coder pays).  Tokens are chosen
 * greedily: at the first position not yet covered, the match if there is one, else the literal.  After a step all of its
 * positions with three bytes behind them enter the table, the highest position winning a bucket.  Nothing depends on lanes() or on
 * the order in which workers store: the device, 64 positions at a time, and the host program, one at a time, write the same bytes.
 *
 * The match pass runs twice and no token is kept: the first pass counts the symbols, from which the three candidates' sizes follow
 * exactly -- stored (5 + n bytes), fixed codes (section 3.2.6), dynamic codes (3.2.7: lengths at most 15, code-length-code
 * lengths at most 7, HLIT / HDIST / HCLEN trimmed) --; the second pass writes the smallest (ties: the lower type) with its codes.
 * The code sets are complete, except that a distance set with one or no symbol in use is one code of one bit, which zlib and
 * lfq_inflate.h accept; the end-of-block symbol always has a code.  Lengths are Huffman's, then limited by moving codes down from
 * the cap until the Kraft sum is one again.
 *
 * Termination: every loop runs over positions, table entries or symbols, or decreases a counter it states.
 */
#ifndef LFQ_DEFLATE_H
#define LFQ_DEFLATE_H

#include <stdint.h>

#include "lfq_inflate.h"

#define LFQ_DEF_MAX_IN 65280            /* htslib's BGZF_BLOCK_SIZE: a stored block of it still fits BSIZE */
#define LFQ_DEF_STEP 64                 /* positions a step */
#define LFQ_DEF_HASH_BITS 12
#define LFQ_DEF_MIN_MATCH 3
#define LFQ_DEF_MAX_MATCH 258
#define LFQ_DEF_MAX_DIST 32768
#define LFQ_DEF_SYM_COST 12             /* bits a match is taken to cost for its length and distance symbols */
#define LFQ_DEF_WIN 100                 /* dwords of the bit window: 31 bits carried + 64 tokens of at most 48 bits */
#define LFQ_DEF_STORED 0
#define LFQ_DEF_FIXED 1
#define LFQ_DEF_DYNAMIC 2

/* the state of one payload in flight (the device keeps it in LDS) */
struct LfqDefState {
    union {
        uint16_t head[1 << LFQ_DEF_HASH_BITS];  /* position + 1 per hash, 0 = none */
        struct {                                /* between the passes: the Huffman construction and the dynamic header */
            uint32_t w[2 * 288];                /* weights of leaves and inner nodes, then depths */
            uint16_t parent[2 * 288];
            uint16_t order[288];                /* symbols in use, by ascending (frequency, symbol) */
            uint16_t rle[288 + 32];             /* code-length symbols: symbol | extra bits' value << 8 */
        } hf;
    };
    uint32_t hist[256];                 /* bytes of the payload */
    uint32_t lfreq[288], dfreq[32], cfreq[19];
    uint16_t lcode[288], dcode[32], ccode[19];  /* bit-reversed: the first bit of the code is bit 0 */
    uint8_t llen[288], dlen[32], clen[19];
    uint32_t cost_sum, n_rle, avg16;
    uint32_t cnt[LFQ_INF_MAXBITS + 1];  /* codes per length while a code is made */
    uint32_t acc[2];                    /* per step: the positions with a match */
    uint16_t hsh[LFQ_DEF_STEP], mlen[LFQ_DEF_STEP], mdist[LFQ_DEF_STEP];
    uint32_t nb[LFQ_DEF_STEP + 1];      /* bits of the step's tokens, then their exclusive prefix sums and the total */
    uint32_t tv_lo[LFQ_DEF_STEP], tv_hi[LFQ_DEF_STEP];
    uint32_t win[LFQ_DEF_WIN];          /* the stream's bits from dword (bit position / 32) on, not yet written */
};

struct LfqDefResult {
    uint32_t n_bytes;                   /* of the stream */
    uint32_t btype;
};

LFQ_INF_FN int lfq_def_log2(uint32_t v) { return 31 - __builtin_clz(v); }      /* v > 0 */

/* 16 log2(v), the mantissa interpolated linearly; 0 < v <= 65536 */
LFQ_INF_FN uint32_t lfq_def_lg16(uint32_t v)
{
    const int b = lfq_def_log2(v);
    return 16u * (uint32_t)b + ((v << 4) >> b) - 16u;
}

LFQ_INF_FN uint32_t lfq_def_hash(uint32_t b0, uint32_t b1, uint32_t b2)
{
    return ((b0 | (b1 << 8) | (b2 << 16)) * 2654435761u) >> (32 - LFQ_DEF_HASH_BITS);
}

/* a match length 3 .. 258: its symbol, the number of extra bits and their value (RFC 1951 section 3.2.5) */
LFQ_INF_FN void lfq_def_len_sym(uint32_t len, uint32_t *sym, uint32_t *xb, uint32_t *xv)
{
    const uint32_t l = len - 3;
    if (len == 258) {
        *sym = 285; *xb = 0; *xv = 0;
    } else if (l < 8) {
        *sym = 257 + l; *xb = 0; *xv = 0;
    } else {
        const int b = lfq_def_log2(l);
        *xb = (uint32_t)b - 2;
        *sym = 257 + 4 * ((uint32_t)b - 1) + ((l >> (b - 2)) & 3u);
        *xv = l & ((1u << (b - 2)) - 1u);
    }
}

/* a distance 1 .. 32768 */
LFQ_INF_FN void lfq_def_dist_sym(uint32_t dist, uint32_t *sym, uint32_t *xb, uint32_t *xv)
{
    const uint32_t d = dist - 1;
    if (d < 4) {
        *sym = d; *xb = 0; *xv = 0;
    } else {
        const int b = lfq_def_log2(d);
        *xb = (uint32_t)b - 1;
        *sym = 2 * (uint32_t)b + ((d >> (b - 1)) & 1u);
        *xv = d & ((1u << (b - 1)) - 1u);
    }
}

LFQ_INF_FN uint32_t lfq_def_lext(uint32_t sym) { return sym < 265 || sym == 285 ? 0u : (sym - 261) >> 2; }  /* sym 257 .. 285 */
LFQ_INF_FN uint32_t lfq_def_dext(uint32_t sym) { return sym < 4 ? 0u : (sym >> 1) - 1u; }                  /* sym 0 .. 29 */

/* Code lengths of at most maxbits for the n symbols with frequencies f[] into len[]; 0 = not in use.  With fewer than two symbols in
 * use the result is one code of one bit (symbol 0 when none is in use) -- and, when `complete`, a second one beside it. */
template <class Io>
LFQ_INF_FN void lfq_def_lengths(LfqDefState *S, const uint32_t *f, int n, int maxbits, bool complete, uint8_t *len, Io &io)
{
    io.sync();
    /* the symbols in use, sorted by (frequency, symbol): each finds its own rank */
    for (int i = io.lane(); i < n; i += io.lanes()) {
        len[i] = 0;
        if (f[i]) {
            int r = 0;
            for (int j = 0; j < n; j++) {
                r += f[j] && (f[j] < f[i] || (f[j] == f[i] && j < i)) ? 1 : 0;
            }
            S->hf.order[r] = (uint16_t)i;
        }
    }
    io.sync();
    if (io.lane() == 0) {
        int m = 0;
        for (int i = 0; i < n; i++) {
            m += f[i] ? 1 : 0;
        }
        if (m < 2) {
            const int s = m ? (int)S->hf.order[0] : 0;
            len[s] = 1;
            if (complete) {
                len[s ? 0 : 1] = 1;
            }
        } else {
            uint32_t *w = S->hf.w;
            uint16_t *par = S->hf.parent;
            for (int k = 0; k < m; k++) {
                w[k] = f[S->hf.order[k]];
            }
            /* Huffman with two queues: the leaves in order, and the inner nodes, which are made in order of weight */
            int leaf = 0, inner = m;
            for (int nxt = m; nxt < 2 * m - 1; nxt++) {
                int pick[2];
                for (int t = 0; t < 2; t++) {
                    pick[t] = leaf < m && (inner >= nxt || w[leaf] <= w[inner]) ? leaf++ : inner++;
                }
                w[nxt] = w[pick[0]] + w[pick[1]];
                par[pick[0]] = par[pick[1]] = (uint16_t)nxt;
            }
            w[2 * m - 2] = 0;                   /* from here on depths: a node's parent has the higher number */
            for (int k = 2 * m - 3; k >= 0; k--) {
                w[k] = w[par[k]] + 1;
            }
            uint32_t *cnt = S->cnt;
            for (int L = 0; L <= LFQ_INF_MAXBITS; L++) {
                cnt[L] = 0;
            }
            for (int k = 0; k < m; k++) {
                cnt[w[k] < (uint32_t)maxbits ? w[k] : (uint32_t)maxbits]++;
            }
            /* the Kraft sum in units of 2^-maxbits; every trip takes one unit off: a code leaves the cap, and a shorter code and
             * it become two codes one bit longer than the shorter one */
            int64_t total = 0;
            for (int L = 1; L <= maxbits; L++) {
                total += (int64_t)cnt[L] << (maxbits - L);
            }
            while (total > ((int64_t)1 << maxbits)) {
                int L = maxbits - 1;
                while (L > 0 && !cnt[L]) {
                    L--;
                }
                if (L == 0 || cnt[maxbits] == 0) {
                    break;                      /* (cannot happen: the excess comes from codes at the cap) */
                }
                cnt[maxbits]--;
                cnt[L]--;
                cnt[L + 1] += 2;
                total--;
            }
            int k = 0;                          /* the rarest symbols get the longest codes */
            for (int L = maxbits; L >= 1; L--) {
                for (uint32_t c = 0; c < cnt[L]; c++) {
                    len[S->hf.order[k++]] = (uint8_t)L;
                }
            }
        }
    }
    io.sync();
}

/* the canonical codes of section 3.2.2 for len[0 .. n), each reversed so that its first bit is bit 0 */
template <class Io>
LFQ_INF_FN void lfq_def_codes(LfqDefState *S, const uint8_t *len, int n, uint16_t *code, Io &io)
{
    io.sync();
    uint32_t *first = S->cnt;                   /* per length: codes of it, then the first code of it */
    if (io.lane() == 0) {
        for (int L = 0; L <= LFQ_INF_MAXBITS; L++) {
            first[L] = 0;
        }
        for (int i = 0; i < n; i++) {
            first[len[i] & 15]++;
        }
        uint32_t c = 0, before = 0;
        for (int L = 1; L <= LFQ_INF_MAXBITS; L++) {
            c = (c + before) << 1;
            before = first[L];
            first[L] = c;
        }
    }
    io.sync();
    for (int i = io.lane(); i < n; i += io.lanes()) {
        const int L = len[i] & 15;
        uint32_t v = 0;
        if (L) {
            uint32_t before = 0;                /* symbols of this length in front of i */
            for (int j = 0; j < i; j++) {
                before += (len[j] & 15) == L ? 1u : 0u;
            }
            v = lfq_inf_rev15(first[L] + before) >> (LFQ_INF_MAXBITS - L);
        }
        code[i] = (uint16_t)v;
    }
    io.sync();
}

/* a serial bit writer for the block header: every worker runs it, worker 0 stores */
struct LfqDefBits {
    uint64_t acc;
    uint32_t n, w;                      /* bits in acc, the next dword of the stream */
};

template <class Io>
LFQ_INF_FN void lfq_def_put(LfqDefBits *B, uint32_t v, uint32_t k, Io &io)      /* k <= 16 */
{
    B->acc |= (uint64_t)v << B->n;
    B->n += k;
    if (B->n >= 32) {
        if (io.lane() == 0) {
            io.out32(B->w, (uint32_t)B->acc);
        }
        B->w++;
        B->acc >>= 32;
        B->n -= 32;
    }
}

/* the run-length form of the dynamic block's hlit + hdist code lengths into S->hf.rle, and its symbols counted in S->cfreq */
LFQ_INF_FN void lfq_def_rle(LfqDefState *S, int hlit, int hdist)
{
    for (int i = 0; i < 19; i++) {
        S->cfreq[i] = 0;
    }
    const int total = hlit + hdist;
    uint32_t m = 0;
    int i = 0;
    while (i < total) {                         /* a run of equal lengths a trip */
        const uint32_t v = i < hlit ? S->llen[i] : S->dlen[i - hlit];
        int run = 1;
        while (i + run < total && (i + run < hlit ? S->llen[i + run] : S->dlen[i + run - hlit]) == v) {
            run++;
        }
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const int r = run < 138 ? run : 138;
                S->hf.rle[m++] = (uint16_t)(18u | ((uint32_t)(r - 11) << 8));
                S->cfreq[18]++;
                run -= r;
            }
            if (run >= 3) {
                S->hf.rle[m++] = (uint16_t)(17u | ((uint32_t)(run - 3) << 8));
                S->cfreq[17]++;
                run = 0;
            }
        } else {
            S->hf.rle[m++] = (uint16_t)v;
            S->cfreq[v]++;
            run--;
            while (run >= 3) {
                const int r = run < 6 ? run : 6;
                S->hf.rle[m++] = (uint16_t)(16u | ((uint32_t)(r - 3) << 8));
                S->cfreq[16]++;
                run -= r;
            }
        }
        for (; run > 0; run--) {
            S->hf.rle[m++] = (uint16_t)v;
            S->cfreq[v]++;
        }
    }
    S->n_rle = m;
}

/* One pass of the matcher over the payload.  emit false: the symbols are counted in S->lfreq / S->dfreq.  emit true: the tokens
 * are written with S->lcode / llen / dcode / dlen behind bit *bitpos_io of the stream, whose started dword is S->win[0]. */
template <class Io>
LFQ_INF_FN void lfq_def_pass(LfqDefState *S, uint32_t n, bool emit, uint32_t *bitpos_io, Io &io)
{
    const int ln = io.lane(), lns = io.lanes();
    io.sync();
    for (int i = ln; i < (1 << LFQ_DEF_HASH_BITS); i += lns) {
        S->head[i] = 0;
    }
    io.sync();
    const uint32_t avg16 = S->avg16;
    uint32_t next = 0, bitpos = emit ? *bitpos_io : 0u;
    for (uint32_t B = 0; B < n; B += LFQ_DEF_STEP) {
        const int cnt = (int)(n - B < LFQ_DEF_STEP ? n - B : LFQ_DEF_STEP);
        if (ln == 0) {
            S->acc[0] = S->acc[1] = 0;
        }
        io.sync();
        /* candidates and their lengths, from the table as the steps in front of this one left it */
        for (int i = ln; i < cnt; i += lns) {
            const uint32_t p = B + (uint32_t)i;
            uint32_t h = 0xffffu, mlen = 0, mdist = 0;
            if (p + 3 <= n) {
                h = lfq_def_hash(io.ld8(p), io.ld8(p + 1), io.ld8(p + 2));
                const uint32_t c = S->head[h];
                if (p >= next && c != 0 && p - (c - 1) <= LFQ_DEF_MAX_DIST) {
                    const uint32_t q = c - 1, cap = n - p < LFQ_DEF_MAX_MATCH ? n - p : LFQ_DEF_MAX_MATCH;
                    uint32_t k = 0;
                    while (k + 4 <= cap) {
                        const uint32_t x = io.ld32(q + k) ^ io.ld32(p + k);
                        if (x) {
                            k += (uint32_t)__builtin_ctz(x) >> 3;
                            break;
                        }
                        k += 4;
                    }
                    if (k + 4 > cap) {          /* (the loop ended at the cap, not at a difference) */
                        while (k < cap && io.ld8(q + k) == io.ld8(p + k)) {
                            k++;
                        }
                    }
                    if (k >= LFQ_DEF_MIN_MATCH) {
                        uint32_t s, lx, dx, xv;
                        lfq_def_len_sym(k, &s, &lx, &xv);
                        lfq_def_dist_sym(p - q, &s, &dx, &xv);
                        if (16u * (LFQ_DEF_SYM_COST + lx + dx) < k * avg16) {
                            mlen = k;
                            mdist = p - q;
                            io.or32(&S->acc[i >> 5], 1u << (i & 31));
                        }
                    }
                }
            }
            S->hsh[i] = (uint16_t)h;
            S->mlen[i] = (uint16_t)mlen;
            S->mdist[i] = (uint16_t)mdist;
        }
        io.sync();
        /* the step's positions enter the table; where several share a bucket the highest stays, whoever stored first */
        for (int trip = 0; trip < LFQ_DEF_STEP; trip++) {
            for (int i = ln; i < cnt; i += lns) {
                const uint32_t h = S->hsh[i], v = B + (uint32_t)i + 1u;
                if (h != 0xffffu && S->head[h] < v) {
                    S->head[h] = (uint16_t)v;
                }
            }
            io.sync();
            bool mine = false;
            for (int i = ln; i < cnt; i += lns) {
                const uint32_t h = S->hsh[i];
                mine = mine || (h != 0xffffu && S->head[h] < B + (uint32_t)i + 1u);
            }
            if (!io.any(mine)) {
                break;
            }
        }
        /* the tokens of the step: every worker walks the same few trips, one per match */
        const uint64_t acc = (uint64_t)S->acc[0] | ((uint64_t)S->acc[1] << 32);
        uint64_t starts = 0;
        uint32_t cur = next > B ? next - B : 0u;
        while (cur < (uint32_t)cnt) {
            const uint64_t m = acc >> cur;
            const uint32_t j = m ? cur + (uint32_t)__builtin_ctzll(m) : (uint32_t)cnt - 1u;
            starts |= (j >= 63 ? ~(uint64_t)0 : (((uint64_t)1 << (j + 1)) - 1u)) & ~(((uint64_t)1 << cur) - 1u);
            cur = j + (m ? (uint32_t)S->mlen[j] : 1u);
        }
        next = B + cur;
        for (int i = ln; i < cnt; i += lns) {
            uint32_t nbits = 0;
            if ((starts >> i) & 1u) {
                const uint32_t len = S->mlen[i];
                uint32_t ls, lx, lv, ds = 0, dx = 0, dv = 0;
                if (len) {
                    lfq_def_len_sym(len, &ls, &lx, &lv);
                    lfq_def_dist_sym(S->mdist[i], &ds, &dx, &dv);
                } else {
                    ls = io.ld8(B + (uint32_t)i);
                    lx = lv = 0;
                }
                if (!emit) {
                    io.add32(&S->lfreq[ls], 1u);
                    if (len) {
                        io.add32(&S->dfreq[ds], 1u);
                    }
                } else {
                    uint64_t v = S->lcode[ls];
                    nbits = S->llen[ls];
                    if (len) {
                        v |= (uint64_t)lv << nbits;
                        nbits += lx;
                        v |= (uint64_t)S->dcode[ds] << nbits;
                        nbits += S->dlen[ds];
                        v |= (uint64_t)dv << nbits;
                        nbits += dx;
                    }
                    S->tv_lo[i] = (uint32_t)v;
                    S->tv_hi[i] = (uint32_t)(v >> 32);
                }
            }
            S->nb[i] = nbits;
        }
        io.sync();
        if (!emit) {
            continue;
        }
        if (ln == 0) {
            uint32_t sum = 0;
            for (int i = 0; i < cnt; i++) {
                const uint32_t t = S->nb[i];
                S->nb[i] = sum;
                sum += t;
            }
            S->nb[LFQ_DEF_STEP] = sum;
        }
        io.sync();
        const uint32_t rem = bitpos & 31u, wbase = bitpos >> 5, total = S->nb[LFQ_DEF_STEP];
        for (int i = ln; i < cnt; i += lns) {
            if ((starts >> i) & 1u) {
                const uint32_t off = rem + S->nb[i], sh = off & 31u;
                const uint64_t v = (uint64_t)S->tv_lo[i] | ((uint64_t)S->tv_hi[i] << 32);   /* at most 48 bits */
                io.or32(&S->win[off >> 5], (uint32_t)(v << sh));
                const uint64_t hi = v >> (32 - sh);         /* the bits behind the first dword */
                if ((uint32_t)hi) {
                    io.or32(&S->win[(off >> 5) + 1], (uint32_t)hi);
                }
                if ((uint32_t)(hi >> 32)) {
                    io.or32(&S->win[(off >> 5) + 2], (uint32_t)(hi >> 32));
                }
            }
        }
        io.sync();
        /* the dwords that are full go out; the started one moves to the window's front */
        const uint32_t full = (rem + total) >> 5;
        for (uint32_t k = (uint32_t)ln; k < full; k += (uint32_t)lns) {
            io.out32(wbase + k, S->win[k]);
        }
        const uint32_t carry = S->win[full];
        io.sync();
        for (uint32_t k = (uint32_t)ln; k <= full; k += (uint32_t)lns) {
            S->win[k] = k == 0 ? carry : 0u;
        }
        io.sync();
        bitpos += total;
    }
    io.sync();
    if (emit) {
        *bitpos_io = bitpos;
    }
}

/* The payload's n bytes as one deflate stream.  The stream's dwords go through io.out32; the bits behind the stream's end in its
 * last dword are 0. */
template <class Io>
LFQ_INF_FN LfqDefResult lfq_deflate(LfqDefState *S, uint32_t n, Io &io)
{
    const int ln = io.lane(), lns = io.lanes();
    LfqDefResult R;
    /* the average cost of a literal */
    io.sync();
    for (int i = ln; i < 256; i += lns) {
        S->hist[i] = 0;
    }
    for (int i = ln; i < 288; i += lns) {
        S->lfreq[i] = 0;
    }
    for (int i = ln; i < 32; i += lns) {
        S->dfreq[i] = 0;
    }
    for (int i = ln; i < LFQ_DEF_WIN; i += lns) {
        S->win[i] = 0;
    }
    if (ln == 0) {
        S->cost_sum = 0;
        S->lfreq[256] = 1;                      /* the end of the block */
        S->llen[286] = S->llen[287] = S->dlen[30] = S->dlen[31] = 0;    /* symbols no block uses */
    }
    io.sync();
    for (uint32_t p = (uint32_t)ln; p < n; p += (uint32_t)lns) {
        io.add32(&S->hist[io.ld8(p)], 1u);
    }
    io.sync();
    const uint32_t lgn = lfq_def_lg16(n);
    for (int i = ln; i < 256; i += lns) {
        const uint32_t f = S->hist[i];
        if (f) {
            const uint32_t c = lgn - lfq_def_lg16(f);
            io.add32(&S->cost_sum, f * (c < 16 ? 16u : c));
        }
    }
    io.sync();
    if (ln == 0) {
        const uint32_t a = S->cost_sum / n;
        S->avg16 = a < 16 ? 16u : a;
    }
    io.sync();
    uint32_t bitpos = 0;
    lfq_def_pass(S, n, false, &bitpos, io);
    /* the fixed block's bits, and the symbols' extra bits, which both kinds pay */
    uint64_t fixed_bits = 3, extra_bits = 0;
    for (int s = 0; s < 286; s++) {
        const uint64_t f = S->lfreq[s];
        fixed_bits += f * (uint64_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
        if (s > 256) {
            extra_bits += f * lfq_def_lext((uint32_t)s);
        }
    }
    for (int s = 0; s < 30; s++) {
        const uint64_t f = S->dfreq[s];
        fixed_bits += f * 5u;
        extra_bits += f * lfq_def_dext((uint32_t)s);
    }
    fixed_bits += extra_bits;
    /* the dynamic block: both codes, the run-length form of their lengths, the code for that */
    lfq_def_lengths(S, S->lfreq, 286, LFQ_INF_MAXBITS, true, S->llen, io);
    lfq_def_lengths(S, S->dfreq, 30, LFQ_INF_MAXBITS, false, S->dlen, io);
    int hlit = 286, hdist = 30;
    while (hlit > 257 && S->llen[hlit - 1] == 0) {
        hlit--;
    }
    while (hdist > 1 && S->dlen[hdist - 1] == 0) {
        hdist--;
    }
    if (ln == 0) {
        lfq_def_rle(S, hlit, hdist);
    }
    io.sync();
    const uint32_t n_rle = S->n_rle;
    lfq_def_lengths(S, S->cfreq, 19, 7, true, S->clen, io);
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int hclen = 19;
    while (hclen > 4 && S->clen[order[hclen - 1]] == 0) {
        hclen--;
    }
    uint64_t dyn_bits = 3 + 5 + 5 + 4 + 3 * (uint64_t)hclen + extra_bits;
    for (int s = 0; s < 19; s++) {
        dyn_bits += (uint64_t)S->cfreq[s] * (uint64_t)(S->clen[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0));
    }
    for (int s = 0; s < 286; s++) {
        dyn_bits += (uint64_t)S->lfreq[s] * S->llen[s];
    }
    for (int s = 0; s < 30; s++) {
        dyn_bits += (uint64_t)S->dfreq[s] * S->dlen[s];
    }
    const uint32_t stored_bytes = 5 + n, fixed_bytes = (uint32_t)((fixed_bits + 7) >> 3), dyn_bytes = (uint32_t)((dyn_bits + 7) >> 3);
    R.btype = LFQ_DEF_STORED;
    R.n_bytes = stored_bytes;
    if (fixed_bytes < R.n_bytes) {
        R.btype = LFQ_DEF_FIXED;
        R.n_bytes = fixed_bytes;
    }
    if (dyn_bytes < R.n_bytes) {
        R.btype = LFQ_DEF_DYNAMIC;
        R.n_bytes = dyn_bytes;
    }
    if (R.btype == LFQ_DEF_STORED) {
        /* 01 | LEN | ~LEN | the payload */
        const uint32_t hdr_lo = 1u | (n << 8) | ((~n & 0xffu) << 24), hdr_hi = (~n >> 8) & 0xffu;
        const uint32_t nd = (stored_bytes + 3) >> 2;
        for (uint32_t w = (uint32_t)ln; w < nd; w += (uint32_t)lns) {
            uint32_t v = 0;
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t at = 4 * w + k;
                v |= (at < 4 ? (hdr_lo >> (8 * at)) & 0xffu : at == 4 ? hdr_hi : at < stored_bytes ? io.ld8(at - 5) : 0u) << (8 * k);
            }
            io.out32(w, v);
        }
        return R;
    }
    LfqDefBits Bw;
    Bw.acc = 0;
    Bw.n = 0;
    Bw.w = 0;
    lfq_def_put(&Bw, 1u | ((uint32_t)R.btype << 1), 3, io);
    if (R.btype == LFQ_DEF_DYNAMIC) {
        lfq_def_codes(S, S->clen, 19, S->ccode, io);
        lfq_def_put(&Bw, (uint32_t)(hlit - 257), 5, io);
        lfq_def_put(&Bw, (uint32_t)(hdist - 1), 5, io);
        lfq_def_put(&Bw, (uint32_t)(hclen - 4), 4, io);
        for (int i = 0; i < hclen; i++) {
            lfq_def_put(&Bw, S->clen[order[i]], 3, io);
        }
        for (uint32_t i = 0; i < n_rle; i++) {
            const uint32_t e = S->hf.rle[i], s = e & 0xffu;
            lfq_def_put(&Bw, S->ccode[s], S->clen[s], io);
            if (s >= 16) {
                lfq_def_put(&Bw, e >> 8, s == 16 ? 2u : s == 17 ? 3u : 7u, io);
            }
        }
    } else {
        io.sync();
        for (int i = ln; i < 288; i += lns) {
            S->llen[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        }
        for (int i = ln; i < 32; i += lns) {
            S->dlen[i] = 5;
        }
        io.sync();
    }
    lfq_def_codes(S, S->llen, 288, S->lcode, io);
    lfq_def_codes(S, S->dlen, 32, S->dcode, io);
    /* the header's last, started dword opens the window (the pass resets the table, and with it hf.rle, which is done with) */
    io.sync();
    if (ln == 0) {
        S->win[0] = (uint32_t)Bw.acc;
    }
    bitpos = 32 * Bw.w + Bw.n;
    lfq_def_pass(S, n, true, &bitpos, io);
    /* the end of the block, and the started dwords */
    const uint32_t rem = bitpos & 31u;
    const uint64_t tail = (uint64_t)S->win[0] | ((uint64_t)S->lcode[256] << rem);
    const uint32_t tail_bits = rem + S->llen[256];
    if (ln == 0) {
        if (tail_bits > 0) {
            io.out32(bitpos >> 5, (uint32_t)tail);
        }
        if (tail_bits > 32) {
            io.out32((bitpos >> 5) + 1, (uint32_t)(tail >> 32));
        }
    }
    bitpos += S->llen[256];
    if ((bitpos + 7) >> 3 != R.n_bytes) {
        R.btype |= 0x80u;                       /* the two passes disagree: never */
    }
    return R;
}

#endif
