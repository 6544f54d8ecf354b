/*
 * lfq_vcf.h -- VCF text as the 2.1.4 binary reads and writes it (lfq_vcf_*, `lofreq vcfset`; the rules: INTEGRATION.md section 14) for
 * the host and for the device.  Each rule of the reference's vcf.c, lofreq_vcfset.c and plp.c is stated here once; lfq_vcf.hip runs them
 * with a lane per 16 bytes, per line, per record and per 16 output bytes, lfq_vcf_check.cpp is the header's stand-alone program for the
 * host compiler (tests/test_vcf_edges.py).  The byte classes are lfq_fasta.h's.
 *
 *   lines      '\n' ends a line; a last line without one counts as if it had one (start[n_lines] = n + 1 then).  chomp strips every
 *              trailing '\r' (utils.c:487-497).  More than LFQ_VCF_MAX_LINE bytes in front of the '\n' (the reference's fgets into
 *              LINE_BUF_SIZE 8192 would split the line) and a NUL anywhere are refused.
 *   header     stream mode (vcf_parse_header, vcf.c:684-720): every line up to and including the first whose first 38 bytes are the
 *              #CHROM .. INFO line (a prefix test), which must be among the first LFQ_VCF_MAX_HEADER_LINES.  Found: the records start
 *              behind it; not found: at line 1, and '#' lines are records like any other (the callers rewind).
 *   records    stream mode (vcf_parse_var_from_line, vcf.c:739-810): split at every tab, empty fields count (strsep); the records END
 *              at the first line with fewer than five fields (every caller's loop stops there).  pos = atol(field 2) - 1, qual = -1
 *              when field 6 starts with '.' or is missing, else atoi; with fewer than eight fields FILTER and INFO are both ".".
 *              Field 9 and everything behind it is kept verbatim.
 *   tabix      (the second file of vcfset): '#' lines are skipped anywhere, every other line needs five fields, one CHROM is one run
 *              with POS not decreasing, POS >= 1, REF not empty, an INFO END= not below POS.
 *   predicates VCF_VAR_PASSES (vcf.h:87) is a PREFIX rule, vcf_var_filtered (vcf.c:315-326) an EXACT one; both exist.
 *              vcf_var_is_indel (vcf.c:328-337), vcf_var_has_info_key (vcf.c:343-390: case-insensitive key, '=' or the token's end).
 *   vcfset     lofreq_vcfset.c:387-411 for a record of file 1, :452-477 for a candidate of file 2 (same CHROM string, same POS).
 *   consumers  INFO's DP / SB / DP4 / AF for `filter` and `uniq` (lfq_vc_info_values), the -S mask (lfq_vc_mask_hit, plp.c:337-399).
 *   writer     vcf_write_var (vcf.c:469-497): POS and QUAL are printed from the parsed values, vcf_var_add_to_info (vcf.c:500-521).
 */
#ifndef LFQ_VCF_H
#define LFQ_VCF_H

#include <stdint.h>

#include "lfq_bed.h"
#include "lfq_fasta.h"

#define LFQ_VCF_MAX_LINE 8190
#define LFQ_VCF_MAX_HEADER_LINES 10000
#define LFQ_VCF_HEADER_PREFIX "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
#define LFQ_VCF_HEADER_PREFIX_LEN 38

/* why a file or a vcfset call is refused (include/lofreq_amd.h has the same values as LFQ_VCF_*); all below 8: the device reports
 * the smallest line * 8 + why */
#define LFQ_VC_OK 0
#define LFQ_VC_LINE_TOO_LONG 1
#define LFQ_VC_NUL 2
#define LFQ_VC_NUMBER 3
#define LFQ_VC_FIELDS 4
#define LFQ_VC_UNSORTED 5
#define LFQ_VC_INTERVAL 6
#define LFQ_VC_MULTIALLELIC 7

#define LFQ_VC_STREAM 0
#define LFQ_VC_TABIX 1

/* the flag byte of a line */
#define LFQ_VC_F_PASSES 1u          /* VCF_VAR_PASSES */
#define LFQ_VC_F_FILTERED 2u        /* vcf_var_filtered */
#define LFQ_VC_F_INDEL_LEN 4u       /* strlen(REF) > 1 || strlen(ALT) > 1 */
#define LFQ_VC_F_INDEL_KEY 8u       /* INFO has the key INDEL */
#define LFQ_VC_F_ALT_COMMA 16u
#define LFQ_VC_F_NUMBER 32u         /* POS or QUAL has more digits than are taken */
#define LFQ_VC_F_HASH 64u           /* the line's first byte is '#' */

#define LFQ_VC_OP_INTERSECT 0
#define LFQ_VC_OP_COMPLEMENT 1
#define LFQ_VC_OP_CONCAT 2

/* what the match of a record of file 1 says */
#define LFQ_VC_K_DROPPED 0          /* --only-snvs / --only-indels: silently */
#define LFQ_VC_K_IGNORED 1          /* --only-passed: counted */
#define LFQ_VC_K_TAKEN 2            /* counted in n_vars1, not written */
#define LFQ_VC_K_WRITTEN 3

#define LFQ_VC_NOFF 10

#if defined(__clang__)
#define LFQ_VC_UNROLL _Pragma("unroll")
#else
#define LFQ_VC_UNROLL
#endif

/* ---- how bytes are fetched: a byte, and the aligned dword around one (the buffer is padded: see lfq_vcf.hip) ---- */
LFQ_FA_FN int lfq_vc_byte(const uint8_t *t, int64_t i) { return t[i]; }
LFQ_FA_FN uint32_t lfq_vc_dword(const uint8_t *t, int64_t a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint32_t *>(t + a);
#else
    return (uint32_t)t[a] | ((uint32_t)t[a + 1] << 8) | ((uint32_t)t[a + 2] << 16) | ((uint32_t)t[a + 3] << 24);
#endif
}

struct LfqVcLine {
    uint16_t off[LFQ_VC_NOFF];      /* off[j], j < nf: where field j + 1 starts in the line; j >= nf: end + 1; off[9]: the chomped end */
    uint8_t nf;                     /* fields, capped at 10 (nothing behind FORMAT's tab is walked) */
    uint8_t flags;
    int32_t qual;
    int64_t pos;
};

/* the parsed file as the rules see it: arrays per LINE; record r is line rec_line[r], or first + r when rec_line is null */
struct LfqVcTab {
    const uint8_t *text;
    int64_t n, n_lines, n_rec, first;
    const int64_t *lstart;          /* [n_lines + 1] */
    const uint16_t *off;            /* [n_lines][10] */
    const uint8_t *nf, *flags;
    const int32_t *qual;
    const int64_t *pos;
    const int64_t *rec_line;
    const int32_t *run_id;          /* [n_rec] the CHROM run of a record */
    const int64_t *run_beg;         /* [n_runs + 1] the first record of every run */
    int64_t n_runs;
};

LFQ_FA_FN int64_t lfq_vc_line_of(const LfqVcTab &T, int64_t r) { return T.rec_line ? T.rec_line[r] : T.first + r; }
LFQ_FA_FN int lfq_vc_fbeg(const uint16_t *off, int j) { return off[j]; }
LFQ_FA_FN int lfq_vc_fend(const uint16_t *off, int j) { return j < 8 ? off[j + 1] - 1 : off[9]; }

/* atol / atoi / strtol on [b, e): blanks, a sign, digits.  *many: more than max_digits digits */
LFQ_FA_FN int64_t lfq_vc_atol(const uint8_t *t, int64_t b, int64_t e, int max_digits, bool *many)
{
    while (b < e && lfq_fa_isspace(lfq_vc_byte(t, b))) {
        b++;
    }
    bool neg = false;
    if (b < e && (lfq_vc_byte(t, b) == '-' || lfq_vc_byte(t, b) == '+')) {
        neg = lfq_vc_byte(t, b) == '-';
        b++;
    }
    int64_t v = 0;
    int nd = 0;
    for (; b < e; b++, nd++) {
        const int ch = lfq_vc_byte(t, b);
        if (ch < '0' || ch > '9') {
            break;
        }
        if (nd >= max_digits) {
            *many = true;
            return 0;
        }
        v = v * 10 + (ch - '0');
    }
    return neg ? -v : v;
}

/* does [b, e) have `key` (upper case, klen bytes) as vcf_var_has_info_key finds it?  *vb, *ve: what follows the token's '=' (vb = -1:
 * the token has none) */
LFQ_FA_FN bool lfq_vc_info_key(const uint8_t *t, int64_t b, int64_t e, const char *key, int klen, int64_t *vb, int64_t *ve)
{
    *vb = -1;
    *ve = -1;
    if (e - b < 2) {
        return false;
    }
    for (int64_t tb = b; tb <= e;) {
        int64_t te = tb;
        while (te < e && lfq_vc_byte(t, te) != ';') {
            te++;
        }
        if (te - tb >= klen) {
            bool same = true;
            for (int i = 0; same && i < klen; i++) {
                int ch = lfq_vc_byte(t, tb + i);
                ch = ch >= 'a' && ch <= 'z' ? ch - 32 : ch;
                same = ch == key[i];
            }
            if (same && (te - tb == klen || lfq_vc_byte(t, tb + klen) == '=')) {
                if (te - tb > klen) {
                    *vb = tb + klen + 1;
                    *ve = te;
                }
                return true;
            }
        }
        tb = te + 1;
    }
    return false;
}

/* line [s, e_raw) of the text (e_raw: its '\n' or the file's end) -> *L.  The tabs come from aligned dwords; nothing outside the
 * dwords around [s, e_raw) is read, and nothing behind INFO's tab */
LFQ_FA_FN void lfq_vc_parse_line(const uint8_t *t, int64_t s, int64_t e_raw, LfqVcLine *L)
{
    int64_t e = e_raw;
    while (e > s && lfq_vc_byte(t, e - 1) == '\r') {
        e--;
    }
    int nt = 0;
    LFQ_VC_UNROLL
    for (int j = 0; j < LFQ_VC_NOFF; j++) {
        L->off[j] = 0;
    }
    for (int64_t a = s & ~(int64_t)3; a < e && nt < 9; a += 4) {
        uint32_t m = lfq_fa_nibble(lfq_fa_eq_hi(lfq_vc_dword(t, a), 0x09));
        if (a < s) {
            m &= 0xfu << (s - a);
        }
        if (a + 4 > e) {
            m &= (1u << (e - a)) - 1u;
        }
        for (; m && nt < 9; m &= m - 1) {        /* (the ninth tab only counts: FORMAT's end; no sample is walked) */
            const uint16_t at = (uint16_t)(a + __builtin_ctz(m) + 1 - s);
            nt++;
            LFQ_VC_UNROLL
            for (int j = 1; j < 9; j++) {           /* (a select per slot: the offsets stay in registers on the device) */
                L->off[j] = j == nt ? at : L->off[j];
            }
        }
    }
    const int nf = nt + 1;
    LFQ_VC_UNROLL
    for (int j = 1; j < 9; j++) {
        L->off[j] = j >= nf ? (uint16_t)(e - s + 1) : L->off[j];
    }
    L->off[9] = (uint16_t)(e - s);
    L->nf = (uint8_t)nf;
    uint32_t fl = s < e && lfq_vc_byte(t, s) == '#' ? LFQ_VC_F_HASH : 0u;
    bool many = false;
    L->pos = nf >= 2 ? lfq_vc_atol(t, s + lfq_vc_fbeg(L->off, 1), s + lfq_vc_fend(L->off, 1), 18, &many) - 1 : -1;
    L->qual = -1;
    if (nf >= 6) {
        const int64_t qb = s + lfq_vc_fbeg(L->off, 5), qe = s + lfq_vc_fend(L->off, 5);
        if (!(qb < qe && lfq_vc_byte(t, qb) == '.')) {
            L->qual = (int32_t)lfq_vc_atol(t, qb, qe, 9, &many);
        }
    }
    fl |= many ? LFQ_VC_F_NUMBER : 0u;
    if (nf >= 5) {
        const int64_t rb = s + lfq_vc_fbeg(L->off, 3), re = s + lfq_vc_fend(L->off, 3), ab = s + lfq_vc_fbeg(L->off, 4),
                      ae = s + lfq_vc_fend(L->off, 4);
        fl |= re - rb > 1 || ae - ab > 1 ? LFQ_VC_F_INDEL_LEN : 0u;
        for (int64_t i = ab; i < ae; i++) {
            if (lfq_vc_byte(t, i) == ',') {
                fl |= LFQ_VC_F_ALT_COMMA;
                break;
            }
        }
    }
    if (nf >= 8) {
        const int64_t fb = s + lfq_vc_fbeg(L->off, 6), fe = s + lfq_vc_fend(L->off, 6);
        const int64_t n = fe - fb;
        const bool dot = n >= 1 && lfq_vc_byte(t, fb) == '.';
        const bool pass = n >= 4 && lfq_vc_byte(t, fb) == 'P' && lfq_vc_byte(t, fb + 1) == 'A' && lfq_vc_byte(t, fb + 2) == 'S'
                          && lfq_vc_byte(t, fb + 3) == 'S';
        fl |= dot || pass ? LFQ_VC_F_PASSES : 0u;
        fl |= (dot && n == 1) || (pass && n == 4) ? 0u : LFQ_VC_F_FILTERED;
        int64_t vb, ve;
        fl |= lfq_vc_info_key(t, s + lfq_vc_fbeg(L->off, 7), s + lfq_vc_fend(L->off, 7), "INDEL", 5, &vb, &ve) ? LFQ_VC_F_INDEL_KEY : 0u;
    } else {
        fl |= LFQ_VC_F_PASSES;          /* FILTER and INFO are "." */
    }
    L->flags = (uint8_t)fl;
}

LFQ_FA_FN bool lfq_vc_is_header_line(const uint8_t *t, int64_t s, int64_t n)
{
    if (s + LFQ_VCF_HEADER_PREFIX_LEN > n) {
        return false;
    }
    const char *want = LFQ_VCF_HEADER_PREFIX;
    for (int i = 0; i < LFQ_VCF_HEADER_PREFIX_LEN; i++) {
        if (lfq_vc_byte(t, s + i) != want[i]) {
            return false;
        }
    }
    return true;
}

LFQ_FA_FN bool lfq_vc_is_indel(uint32_t fl) { return (fl & (LFQ_VC_F_INDEL_LEN | LFQ_VC_F_INDEL_KEY)) != 0; }

/* the INFO field of line k: [*b, *e); false: the line has fewer than eight fields and its INFO is "." */
LFQ_FA_FN bool lfq_vc_info_range(const LfqVcTab &T, int64_t k, int64_t *b, int64_t *e)
{
    const uint16_t *off = T.off + k * LFQ_VC_NOFF;
    *b = T.lstart[k] + lfq_vc_fbeg(off, 7);
    *e = T.lstart[k] + lfq_vc_fend(off, 7);
    return T.nf[k] >= 8;
}

/* a tabix-mode record on its own: POS >= 1, REF not empty, END= not below POS */
LFQ_FA_FN bool lfq_vc_interval_ok(const LfqVcTab &T, int64_t k)
{
    const uint16_t *off = T.off + k * LFQ_VC_NOFF;
    if (T.pos[k] < 0 || lfq_vc_fend(off, 3) - lfq_vc_fbeg(off, 3) < 1) {
        return false;
    }
    int64_t b, e, vb, ve;
    if (lfq_vc_info_range(T, k, &b, &e) && lfq_vc_info_key(T.text, b, e, "END", 3, &vb, &ve) && vb >= 0) {
        bool many = false;
        const int64_t end = lfq_vc_atol(T.text, vb, ve, 18, &many);
        return many || end >= T.pos[k] + 1;
    }
    return true;
}

/* field j of line ka of A and of line kb of B: the same bytes? */
LFQ_FA_FN bool lfq_vc_field_equal(const LfqVcTab &A, int64_t ka, const LfqVcTab &B, int64_t kb, int j)
{
    const uint16_t *oa = A.off + ka * LFQ_VC_NOFF, *ob = B.off + kb * LFQ_VC_NOFF;
    const int64_t a = A.lstart[ka] + lfq_vc_fbeg(oa, j), na = lfq_vc_fend(oa, j) - lfq_vc_fbeg(oa, j);
    const int64_t b = B.lstart[kb] + lfq_vc_fbeg(ob, j), nb = lfq_vc_fend(ob, j) - lfq_vc_fbeg(ob, j);
    if (na != nb) {
        return false;
    }
    for (int64_t i = 0; i < na; i++) {
        if (lfq_vc_byte(A.text, a + i) != lfq_vc_byte(B.text, b + i)) {
            return false;
        }
    }
    return true;
}

struct LfqVcSetConf {
    int op, only_passed, only_pos, only_snvs, only_indels;
};

/* the tests of a record of file 1 in the reference's order (lofreq_vcfset.c:387-411): LFQ_VC_K_DROPPED, LFQ_VC_K_IGNORED, -1 = the
 * call is refused (multi-allelic), or LFQ_VC_K_TAKEN */
LFQ_FA_FN int lfq_vc_var1(uint32_t fl, const LfqVcSetConf &c)
{
    const bool indel = lfq_vc_is_indel(fl);
    if ((c.only_snvs && indel) || (c.only_indels && !indel)) {
        return LFQ_VC_K_DROPPED;
    }
    if (!c.only_pos && (fl & LFQ_VC_F_ALT_COMMA)) {
        return -1;
    }
    if (c.only_passed && !(fl & LFQ_VC_F_PASSES)) {
        return LFQ_VC_K_IGNORED;
    }
    return LFQ_VC_K_TAKEN;
}

/* does line ka of file 1 have a match in run `run` of file 2 (-1: file 2 lacks the CHROM)?  lofreq_vcfset.c:452-477 */
LFQ_FA_FN bool lfq_vc_match(const LfqVcTab &A, int64_t ka, const LfqVcTab &B, int64_t run, const LfqVcSetConf &c)
{
    if (run < 0) {
        return false;
    }
    const int64_t p = A.pos[ka], r1 = B.run_beg[run + 1];
    int64_t lo = B.run_beg[run], hi = r1;       /* -> the first record of the run with pos >= p */
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (B.pos[lfq_vc_line_of(B, mid)] < p) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    for (int64_t r = lo; r < r1; r++) {
        const int64_t kb = lfq_vc_line_of(B, r);
        if (B.pos[kb] != p) {
            break;
        }
        const uint32_t fl = B.flags[kb];
        const bool indel = lfq_vc_is_indel(fl);
        if ((c.only_passed && !(fl & LFQ_VC_F_PASSES)) || (c.only_snvs && indel) || (c.only_indels && !indel)) {
            continue;
        }
        if (c.only_pos || (lfq_vc_field_equal(A, ka, B, kb, 3) && lfq_vc_field_equal(A, ka, B, kb, 4))) {
            return true;
        }
    }
    return false;
}

/* ---- the writer: a written line is nine pieces; LfqVcPieces says how long each is and where its bytes come from ---- */
LFQ_FA_FN int lfq_vc_ndigits(int64_t v)         /* the bytes of %ld */
{
    int n = v < 0 ? 2 : 1;
    for (uint64_t u = v < 0 ? (uint64_t)(-v) : (uint64_t)v; u >= 10; u /= 10) {
        n++;
    }
    return n;
}
LFQ_FA_FN int lfq_vc_digit_at(int64_t v, int nd, int i)
{
    if (v < 0 && i == 0) {
        return '-';
    }
    uint64_t u = v < 0 ? (uint64_t)(-v) : (uint64_t)v;
    for (int k = nd - 1; k > i; k--) {
        u /= 10;
    }
    return '0' + (int)(u % 10);
}

struct LfqVcPieces {
    int64_t s;                      /* the line's start in the text */
    int32_t len[9], src[9];         /* src: where a verbatim piece starts in the line; -1: made */
    int32_t total;
    int64_t pos1;                   /* POS as written */
    int32_t qual;
};

/* add_len: the bytes of the --add-info string, 0: none */
LFQ_FA_FN void lfq_vc_pieces(const LfqVcTab &T, int64_t k, int add_len, LfqVcPieces *P)
{
    const uint16_t *off = T.off + k * LFQ_VC_NOFF;
    const int nf = T.nf[k];
    P->s = T.lstart[k];
    P->pos1 = T.pos[k] + 1;
    P->qual = T.qual[k];
    P->src[0] = 0;                  P->len[0] = off[1];                                     /* CHROM and its tab */
    P->src[1] = -1;                 P->len[1] = lfq_vc_ndigits(P->pos1);                    /* POS */
    P->src[2] = off[2] - 1;         P->len[2] = lfq_vc_fend(off, 4) - (off[2] - 1);         /* tab ID tab REF tab ALT */
    P->src[3] = -1;                 P->len[3] = 1 + (P->qual > -1 ? lfq_vc_ndigits(P->qual) : 1);   /* tab QUAL */
    const int info_len = nf >= 8 ? lfq_vc_fend(off, 7) - lfq_vc_fbeg(off, 7) : 1;
    const bool info_dot = nf < 8 || (info_len == 1 && lfq_vc_byte(T.text, P->s + off[7]) == '.');
    if (nf >= 8) {
        P->src[4] = off[6] - 1;     P->len[4] = off[7] - (off[6] - 1);                      /* tab FILTER tab */
    } else {
        P->src[4] = -1;             P->len[4] = 3;                                          /* tab . tab */
    }
    const bool keep_info = add_len == 0 || !(info_dot || info_len == 0);
    P->src[5] = nf >= 8 ? (int32_t)off[7] : -1;
    P->len[5] = keep_info ? info_len : 0;
    P->src[6] = -1;                 P->len[6] = add_len == 0 ? 0 : add_len + (P->len[5] > 0 ? 1 : 0);   /* ; and the string */
    P->src[7] = nf >= 9 ? off[8] - 1 : -1;
    P->len[7] = nf >= 9 ? off[9] - (off[8] - 1) : 0;                                        /* tab FORMAT and the samples */
    P->src[8] = -1;                 P->len[8] = 1;
    int32_t total = 0;
    for (int i = 0; i < 9; i++) {
        total += P->len[i];
    }
    P->total = total;
}

/* byte q of the written line, 0 <= q < total */
LFQ_FA_FN int lfq_vc_piece_byte(const LfqVcTab &T, const LfqVcPieces &P, int32_t q, const char *add)
{
    int i = 8, src = -1;
    bool found = false;
    LFQ_VC_UNROLL
    for (int j = 0; j < 9; j++) {       /* (unrolled: the pieces stay in registers) */
        if (!found && q < P.len[j]) {
            found = true;
            i = j;
            src = P.src[j];
        }
        q -= found ? 0 : P.len[j];
    }
    if (src >= 0) {
        return lfq_vc_byte(T.text, P.s + src + q);
    }
    switch (i) {
    case 1:
        return lfq_vc_digit_at(P.pos1, P.len[1], q);
    case 3:
        return q == 0 ? '\t' : P.qual > -1 ? lfq_vc_digit_at(P.qual, P.len[3] - 1, q - 1) : '.';
    case 4:
        return q == 1 ? '.' : '\t';
    case 5:
        return '.';
    case 6:
        return P.len[5] > 0 ? (q == 0 ? ';' : add[q - 1]) : add[q];
    default:
        return '\n';
    }
}

/* the keys `lofreq filter` and `lofreq uniq` read, in one walk per key of INFO (vcf_get_dp4: vcf.c:566-604) */
struct LfqVcInfo {
    int32_t dp, sb, dp4[4];
    int32_t has;                    /* bit 0 DP, 1 SB, 2 DP4 (four fields), 3 AF */
    int32_t af_len;
    int64_t af_beg;                 /* in the text */
};
LFQ_FA_FN void lfq_vc_info_values(const LfqVcTab &T, int64_t k, LfqVcInfo *I)
{
    I->dp = 0;
    I->sb = 0;
    I->dp4[0] = I->dp4[1] = I->dp4[2] = I->dp4[3] = -1;
    I->has = 0;
    I->af_len = 0;
    I->af_beg = 0;
    int64_t b, e, vb, ve;
    if (!lfq_vc_info_range(T, k, &b, &e)) {
        return;
    }
    bool many = false;
    if (lfq_vc_info_key(T.text, b, e, "DP", 2, &vb, &ve)) {
        I->has |= 1;
        I->dp = vb >= 0 ? (int32_t)lfq_vc_atol(T.text, vb, ve, 18, &many) : 0;
    }
    if (lfq_vc_info_key(T.text, b, e, "SB", 2, &vb, &ve)) {
        I->has |= 2;
        I->sb = vb >= 0 ? (int32_t)lfq_vc_atol(T.text, vb, ve, 18, &many) : 0;
    }
    if (lfq_vc_info_key(T.text, b, e, "DP4", 3, &vb, &ve) && vb >= 0) {
        int nfld = 0;
        int32_t v[4] = {-1, -1, -1, -1};
        for (int64_t fb = vb; fb <= ve; nfld++) {
            int64_t fe = fb;
            while (fe < ve && lfq_vc_byte(T.text, fe) != ',') {
                fe++;
            }
            if (nfld < 4) {
                v[nfld] = (int32_t)lfq_vc_atol(T.text, fb, fe, 18, &many);
            }
            fb = fe + 1;
        }
        if (nfld == 4) {
            I->has |= 4;
            for (int i = 0; i < 4; i++) {
                I->dp4[i] = v[i];
            }
        }
    }
    if (lfq_vc_info_key(T.text, b, e, "AF", 2, &vb, &ve) && vb >= 0) {
        I->has |= 8;
        I->af_beg = vb;
        I->af_len = (int32_t)(ve - vb);
    }
}

/* -S / --ign-vcf (source_qual_load_ign_vcf, plp.c:337-399): a record of the named CHROM marks its position when that lies on the contig
 * and, under a BED, [pos, pos + 1) overlaps the table of that name (plp.c:376).  bed.n < 0: no BED */
LFQ_FA_FN bool lfq_vc_mask_hit(int64_t pos, int64_t ref_len, const LfqBedTab &bed)
{
    return pos >= 0 && pos < ref_len && (bed.n < 0 || lfq_bed_tab_overlap(bed, pos, pos + 1));
}

/* ---- host only from here on: the same rules, one thread, line by line (what the kernels of lfq_vcf.hip compute) ---- */
struct LfqVcHostFile {
    std::vector<uint8_t> text;          /* padded with zeros to a multiple of 16 plus 16, as the device buffer */
    int64_t n = 0, n_lines = 0, n_rec = 0, first = 0, hdr_line = -1, lines_behind = 0;
    int mode = LFQ_VC_STREAM;
    std::vector<int64_t> lstart, pos, rec_line, run_beg;
    std::vector<uint16_t> off;
    std::vector<uint8_t> nf, flags;
    std::vector<int32_t> qual, run_id;
    std::vector<std::string> run_name;
    LfqVcTab tab() const
    {
        LfqVcTab T;
        T.text = text.data(); T.n = n; T.n_lines = n_lines; T.n_rec = n_rec; T.first = first;
        T.lstart = lstart.data(); T.off = off.data(); T.nf = nf.data(); T.flags = flags.data(); T.qual = qual.data(); T.pos = pos.data();
        T.rec_line = mode == LFQ_VC_TABIX ? rec_line.data() : nullptr;
        T.run_id = run_id.data(); T.run_beg = run_beg.data(); T.n_runs = (int64_t)run_name.size();
        return T;
    }
};

/* LFQ_VC_OK, or why the file is refused and at which line (1-based): the smallest line * 8 + why over all offences */
static inline int lfq_vc_host_open(const uint8_t *bytes, int64_t n, int mode, LfqVcHostFile *F, int64_t *bad_line)
{
    *F = LfqVcHostFile();
    *bad_line = 0;
    F->mode = mode;
    F->n = n;
    if (n <= 0) {
        F->run_beg.push_back(0);
        return LFQ_VC_OK;
    }
    F->text.assign((size_t)((n + 15) / 16 * 16 + 16), 0);
    std::copy(bytes, bytes + n, F->text.begin());
    lfq_fa_host_lines(bytes, n, &F->lstart);
    F->n_lines = (int64_t)F->lstart.size() - 1;
    const int64_t nl = F->n_lines;
    uint64_t bad = UINT64_MAX;
    auto offend = [&](int64_t line, int why) { bad = std::min(bad, (uint64_t)line * 8 + (uint64_t)why); };
    F->off.assign((size_t)nl * LFQ_VC_NOFF, 0);
    F->nf.assign((size_t)nl, 0);
    F->flags.assign((size_t)nl, 0);
    F->qual.assign((size_t)nl, -1);
    F->pos.assign((size_t)nl, -1);
    const uint8_t *t = F->text.data();
    for (int64_t k = 0; k < nl; k++) {
        const int64_t s = F->lstart[(size_t)k], e = F->lstart[(size_t)k + 1] - 1;
        for (int64_t i = s; i < e; i++) {
            if (t[i] == 0) {
                offend(k, LFQ_VC_NUL);
                break;
            }
        }
        if (e - s > LFQ_VCF_MAX_LINE) {
            offend(k, LFQ_VC_LINE_TOO_LONG);
            continue;
        }
        if (mode == LFQ_VC_STREAM && F->hdr_line < 0 && k < LFQ_VCF_MAX_HEADER_LINES && lfq_vc_is_header_line(t, s, n)) {
            F->hdr_line = k;
        }
        LfqVcLine L;
        lfq_vc_parse_line(t, s, e, &L);
        std::copy(L.off, L.off + LFQ_VC_NOFF, F->off.begin() + (size_t)k * LFQ_VC_NOFF);
        F->nf[(size_t)k] = L.nf; F->flags[(size_t)k] = L.flags; F->qual[(size_t)k] = L.qual; F->pos[(size_t)k] = L.pos;
    }
    if (mode == LFQ_VC_STREAM) {
        F->first = F->hdr_line + 1;
        int64_t end = F->first;
        while (end < nl && F->nf[(size_t)end] >= 5 && F->lstart[(size_t)end + 1] - 1 - F->lstart[(size_t)end] <= LFQ_VCF_MAX_LINE) {
            end++;
        }
        F->n_rec = end - F->first;
        F->lines_behind = nl - end;
    } else {
        for (int64_t k = 0; k < nl; k++) {
            if (F->flags[(size_t)k] & LFQ_VC_F_HASH || F->lstart[(size_t)k + 1] - 1 - F->lstart[(size_t)k] > LFQ_VCF_MAX_LINE) {
                continue;
            }
            if (F->nf[(size_t)k] < 5) {
                offend(k, LFQ_VC_FIELDS);
                continue;
            }
            F->rec_line.push_back(k);
        }
        F->n_rec = (int64_t)F->rec_line.size();
    }
    LfqVcTab T = F->tab();
    F->run_id.assign((size_t)F->n_rec, 0);
    for (int64_t r = 0; r < F->n_rec; r++) {
        const int64_t k = lfq_vc_line_of(T, r), kp = r > 0 ? lfq_vc_line_of(T, r - 1) : -1;
        if (F->flags[(size_t)k] & LFQ_VC_F_NUMBER) {
            offend(k, LFQ_VC_NUMBER);
        }
        const bool head = r == 0 || !lfq_vc_field_equal(T, k, T, kp, 0);
        if (head) {
            F->run_beg.push_back(r);
            F->run_name.emplace_back((const char *)t + F->lstart[(size_t)k], (size_t)lfq_vc_fend(T.off + k * LFQ_VC_NOFF, 0));
        }
        F->run_id[(size_t)r] = (int32_t)F->run_name.size() - 1;
        if (mode == LFQ_VC_TABIX) {
            if (!lfq_vc_interval_ok(T, k)) {
                offend(k, LFQ_VC_INTERVAL);
            }
            if (!head && F->pos[(size_t)k] < F->pos[(size_t)kp]) {
                offend(k, LFQ_VC_UNSORTED);
            }
        }
    }
    F->run_beg.push_back(F->n_rec);
    if (mode == LFQ_VC_TABIX && bad == UINT64_MAX) {      /* one run per name: the later run's first record offends */
        for (size_t i = 0; i < F->run_name.size(); i++) {
            for (size_t j = 0; j < i; j++) {
                if (F->run_name[i] == F->run_name[j]) {
                    offend(lfq_vc_line_of(T, F->run_beg[i]), LFQ_VC_UNSORTED);
                }
            }
        }
    }
    if (bad != UINT64_MAX) {
        *bad_line = (int64_t)(bad / 8) + 1;
        return (int)(bad % 8);
    }
    return LFQ_VC_OK;
}

/* file 1's runs -> file 2's by name; -1: file 2 lacks the CHROM */
static inline std::vector<int64_t> lfq_vc_run_map(const std::vector<std::string> &a, const std::vector<std::string> &b)
{
    std::vector<int64_t> m(a.size(), -1);
    for (size_t i = 0; i < a.size(); i++) {
        for (size_t j = 0; j < b.size(); j++) {
            if (a[i] == b[j]) {
                m[i] = (int64_t)j;
                break;
            }
        }
    }
    return m;
}

struct LfqVcSetOut {
    int64_t n_vars1 = 0, n_ignored = 0, n_out = 0;
    int why = LFQ_VC_OK, bad_file = 0;
    int64_t bad_line = 0;
    std::vector<uint8_t> keep;          /* of file 1 (concat: of every file in turn) */
    std::string text;
};

/* vcfset over opened files: files[0] is file 1, `two` file 2 (null for concat, whose further files follow in `files`) */
static inline void lfq_vc_host_set(const std::vector<const LfqVcHostFile *> &files, const LfqVcHostFile *two, const LfqVcSetConf &c,
                                   const std::string &add, bool count_only, LfqVcSetOut *out)
{
    *out = LfqVcSetOut();
    const LfqVcHostFile &one = *files[0];
    if (one.hdr_line >= 0 && !count_only) {
        out->text.assign((const char *)one.text.data(), (size_t)std::min(one.lstart[(size_t)one.hdr_line + 1], one.n));   /* as read */
    }
    const size_t n_files = c.op == LFQ_VC_OP_CONCAT ? files.size() : 1;
    uint64_t bad = UINT64_MAX;
    std::string lines;
    for (size_t f = 0; f < n_files && bad == UINT64_MAX; f++) {
        const LfqVcHostFile &A = *files[f];
        const LfqVcTab TA = A.tab();
        LfqVcTab TB = TA;
        std::vector<int64_t> map;
        if (c.op != LFQ_VC_OP_CONCAT) {
            TB = two->tab();
            map = lfq_vc_run_map(A.run_name, two->run_name);
        }
        for (int64_t r = 0; r < A.n_rec; r++) {
            const int64_t k = lfq_vc_line_of(TA, r);
            int code = lfq_vc_var1(A.flags[(size_t)k], c);
            if (code < 0) {
                bad = std::min(bad, ((uint64_t)f << 40 | (uint64_t)k) * 8 + LFQ_VC_MULTIALLELIC);
                code = LFQ_VC_K_DROPPED;
            } else if (code == LFQ_VC_K_TAKEN && c.op != LFQ_VC_OP_CONCAT && A.pos[(size_t)k] < 0) {
                bad = std::min(bad, ((uint64_t)f << 40 | (uint64_t)k) * 8 + LFQ_VC_INTERVAL);
            } else if (code == LFQ_VC_K_TAKEN) {
                const bool m = c.op == LFQ_VC_OP_CONCAT || lfq_vc_match(TA, k, TB, map[(size_t)A.run_id[(size_t)r]], c) == (c.op == LFQ_VC_OP_INTERSECT);
                code = m ? LFQ_VC_K_WRITTEN : LFQ_VC_K_TAKEN;
            }
            out->keep.push_back((uint8_t)code);
            out->n_ignored += code == LFQ_VC_K_IGNORED;
            out->n_vars1 += code >= LFQ_VC_K_TAKEN;
            out->n_out += code == LFQ_VC_K_WRITTEN;
            if (code == LFQ_VC_K_WRITTEN && !count_only) {
                LfqVcPieces P;
                lfq_vc_pieces(TA, k, (int)add.size(), &P);
                for (int32_t q = 0; q < P.total; q++) {
                    lines.push_back((char)lfq_vc_piece_byte(TA, P, q, add.c_str()));
                }
            }
        }
    }
    if (bad != UINT64_MAX) {
        *out = LfqVcSetOut();
        out->why = (int)(bad % 8);
        out->bad_file = (int)((bad / 8) >> 40);
        out->bad_line = (int64_t)((bad / 8) & (((uint64_t)1 << 40) - 1)) + 1;
        return;
    }
    out->text += lines;
}

#endif
