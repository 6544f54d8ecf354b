/*
 * lfq_fasta.h -- `lofreq faidx` and the contig of a FASTA (lfq_fasta_*; the rules: INTEGRATION.md
 * section 9) for the host and for the device.  The rules of htslib's fai_build_core and fai_retrieve as the 2.1.4 binary applies
 * them (tests/golden/fasta_binary.json) are stated here once; lfq_fasta.hip runs them with a lane per 16 bytes, per line, per header
 * and per 16 bases, lfq_fasta_check.cpp is the header's stand-alone program for the host compiler (tests/test_fasta_edges.py).
 *
 *   bytes      '\n' ends a line; graph bytes (isgraph of the C locale, 0x21 .. 0x7e) are the sequence; every other byte only counts
 *              towards a line's length.  A chunk is 16 aligned bytes: its newline, graph and '>' masks come from its four dwords.
 *   lines      line k is [start[k], start[k + 1]) INCLUDING its terminator; a last line without '\n' counts as if it had one (the
 *              sentinel start[n_lines] is n_bytes + 1 then).  A line is a header iff its first byte is '>'.
 *   sequence   the lines behind a header up to the next one.  Its first line sets line_len (bytes) and line_blen (graph bytes).  A
 *              line is FULL when it has line_len bytes and is not the empty line; the sequence's lines are read as such up to and
 *              including its first line m that is not full (shorter: fine; longer: "Different line length"), and behind m only
 *              "\n" and "\r\n" may stand before the next header ("Format error, unexpected").  Text in front of the first header
 *              is held to the same rule with m in front of it.
 *              That is a chain, not a look at the line before: "\r\n" has the bytes of a full line of a sequence one base wide,
 *              so whether such a line still belongs to the sequence depends on every line since the header.  The device finds m
 *              per sequence with an atomic min in a launch of its own and the first offending line of the file with another.
 *   entries    a header whose next line is missing, empty or another header has no sequence: dropped in mid-file, the whole file
 *              refused when it is the last.  length = the graph bytes of the lines up to m, offset = the first line's first byte.
 *   name       the bytes behind '>' after leading blanks up to the next blank; may be empty.  The first of equal names wins.
 *   fetch      the `length` graph bytes at or behind `offset`, in file order, case kept.  When every line of the span but the last
 *              is line_blen graph bytes and '\n', base p lies at offset + p / line_blen * line_len + p % line_blen.
 */
#ifndef LFQ_FASTA_H
#define LFQ_FASTA_H

#include <stdint.h>

#if defined(__HIPCC__)
#define LFQ_FA_FN __host__ __device__ static inline
#else
#define LFQ_FA_FN static inline
#endif

/* geometry of the scan kernels: a lane owns one chunk, a workgroup one tile of LFQ_FA_THREADS chunks; the scan over the tiles'
 * sums is one wavefront that takes LFQ_FA_SCAN_LANES tiles a round */
#define LFQ_FA_CHUNK 16
#define LFQ_FA_THREADS 256
#define LFQ_FA_SCAN_LANES 64
#define LFQ_FA_TILE (LFQ_FA_THREADS * LFQ_FA_CHUNK)

/* why lfq_fasta_index_build refuses a file (include/lofreq_amd.h has the same values as LFQ_FASTA_*) */
#define LFQ_FA_OK 0
#define LFQ_FA_UNEXPECTED 1
#define LFQ_FA_LINE_LENGTH 2
#define LFQ_FA_LAST_EMPTY 3
#define LFQ_FA_EMPTY_FILE 4

/* ---- byte classes, four bytes at a time: bit 7 of every byte of the result that is in the class ---- */
LFQ_FA_FN uint32_t lfq_fa_eq_hi(uint32_t w, uint32_t byte)
{
    const uint32_t x = w ^ (byte * 0x01010101u);
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;     /* exact: no carry leaves a byte */
}
LFQ_FA_FN uint32_t lfq_fa_graph_hi(uint32_t w)
{
    const uint32_t lo = w & 0x7f7f7f7fu;                                /* 0x21 <= b <= 0x7e and b < 0x80 */
    return (lo + 0x5f5f5f5fu) & ~(lo + 0x01010101u) & ~w & 0x80808080u;
}
LFQ_FA_FN uint32_t lfq_fa_nibble(uint32_t hi)                           /* bits 7, 15, 23, 31 -> bits 0 .. 3 */
{
    const uint32_t m = hi >> 7;
    return (m | (m >> 7) | (m >> 14) | (m >> 21)) & 0xfu;
}
struct LfqFaMasks {
    uint32_t nl, graph, gt;             /* bit i: byte i of the chunk is '\n' / a graph byte / '>' */
};
LFQ_FA_FN LfqFaMasks lfq_fa_chunk_masks(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
{
    LfqFaMasks m;
    m.nl = lfq_fa_nibble(lfq_fa_eq_hi(w0, 0x0a)) | (lfq_fa_nibble(lfq_fa_eq_hi(w1, 0x0a)) << 4)
           | (lfq_fa_nibble(lfq_fa_eq_hi(w2, 0x0a)) << 8) | (lfq_fa_nibble(lfq_fa_eq_hi(w3, 0x0a)) << 12);
    m.graph = lfq_fa_nibble(lfq_fa_graph_hi(w0)) | (lfq_fa_nibble(lfq_fa_graph_hi(w1)) << 4)
              | (lfq_fa_nibble(lfq_fa_graph_hi(w2)) << 8) | (lfq_fa_nibble(lfq_fa_graph_hi(w3)) << 12);
    m.gt = lfq_fa_nibble(lfq_fa_eq_hi(w0, 0x3e)) | (lfq_fa_nibble(lfq_fa_eq_hi(w1, 0x3e)) << 4)
           | (lfq_fa_nibble(lfq_fa_eq_hi(w2, 0x3e)) << 8) | (lfq_fa_nibble(lfq_fa_eq_hi(w3, 0x3e)) << 12);
    return m;
}
/* the newlines of chunk `c` of a file of n bytes that START A LINE (one stands behind them): the file's last byte starts none */
LFQ_FA_FN uint32_t lfq_fa_line_starts(uint32_t nl, int64_t c, int64_t n)
{
    const int64_t last = n - 1 - c * LFQ_FA_CHUNK;
    return last >= 0 && last < LFQ_FA_CHUNK ? nl & ~(1u << last) : nl;
}
LFQ_FA_FN bool lfq_fa_isspace(int ch) { return ch == ' ' || (ch >= '\t' && ch <= '\r'); }
LFQ_FA_FN bool lfq_fa_isgraph(int ch) { return ch >= 0x21 && ch <= 0x7e; }

/* ---- lines ---- */
/* `bytes` counts the terminator: the empty line has 1 */
LFQ_FA_FN bool lfq_fa_line_full(int64_t bytes, int64_t first_bytes) { return bytes != 1 && bytes == first_bytes; }
/* what may stand between a sequence's end and the next header: "\n" and "\r\n" (b1: the line's second byte, -1 when the file ends) */
LFQ_FA_FN bool lfq_fa_line_skippable(int64_t bytes, int b0, int b1) { return bytes == 1 || (bytes == 2 && b0 == '\r' && b1 == '\n'); }
/* non-header line k of a sequence whose first line has first_bytes and whose first line that is not full is m (none: any m > k;
 * text in front of the first header: m < k) -> LFQ_FA_OK or why the file is refused AT THIS LINE */
LFQ_FA_FN int lfq_fa_line_offence(int64_t k, int64_t m, int64_t bytes, int64_t first_bytes, bool skippable)
{
    if (k < m) {
        return LFQ_FA_OK;
    }
    if (k == m) {
        return bytes > first_bytes ? LFQ_FA_LINE_LENGTH : LFQ_FA_OK;
    }
    return skippable ? LFQ_FA_OK : LFQ_FA_UNEXPECTED;
}
/* the name of the header line text[beg, end) (beg: behind '>', end: its '\n' or the file's end) -> [*nb, *nb + *nl) */
LFQ_FA_FN void lfq_fa_name_cut(const uint8_t *text, int64_t beg, int64_t end, int64_t *nb, int64_t *nl)
{
    while (beg < end && lfq_fa_isspace(text[beg])) {
        beg++;
    }
    int64_t e = beg;
    while (e < end && !lfq_fa_isspace(text[e])) {
        e++;
    }
    *nb = beg;
    *nl = e - beg;
}
/* the source byte of base p of a regular sequence */
LFQ_FA_FN int64_t lfq_fa_regular_src(int64_t offset, int64_t p, int64_t blen, int64_t llen) { return offset + p / blen * llen + p % blen; }

/* one header as the device (lfq_fasta_entries_kernel) and the host (below) report it, before names are cut out and duplicates go */
struct LfqFaRaw {
    int64_t length, offset;
    int64_t name_beg;                   /* in the file */
    int32_t line_blen, line_len, name_len;
    int32_t valid;                      /* 0: no sequence line behind the header */
};

/* ---- host only from here on ---- */
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

struct LfqFaEntry {
    std::string name;
    int64_t length, offset;
    int32_t line_blen, line_len;
};

struct lfq_fasta_index {
    std::vector<LfqFaEntry> e;          /* in file order */
    int64_t n_dup = 0;                  /* entries ignored because an earlier one has their name */
    std::string text;                   /* the .fai, made on first request */
    int64_t find(const char *name) const
    {
        for (size_t i = 0; name && i < e.size(); i++) {
            if (e[i].name == name) {
                return (int64_t)i;
            }
        }
        return -1;
    }
};

/* raw entries in file order + their names -> the index.  LFQ_FA_OK, or why the file is refused as a whole (the line rules have
 * been passed by then) */
static inline int lfq_fa_entries_finish(const std::vector<LfqFaRaw> &raw, const std::vector<std::string> &names, lfq_fasta_index *idx)
{
    idx->e.clear();
    idx->n_dup = 0;
    idx->text.clear();
    if (raw.empty()) {
        return LFQ_FA_EMPTY_FILE;       /* (nothing but empty lines is no FASTA either) */
    }
    if (!raw.back().valid) {
        return LFQ_FA_LAST_EMPTY;
    }
    for (size_t h = 0; h < raw.size(); h++) {
        if (!raw[h].valid) {
            continue;
        }
        if (idx->find(names[h].c_str()) >= 0) {
            idx->n_dup++;
            continue;
        }
        idx->e.push_back({names[h], raw[h].length, raw[h].offset, raw[h].line_blen, raw[h].line_len});
    }
    return LFQ_FA_OK;
}

static inline const std::string &lfq_fa_index_text(lfq_fasta_index *idx)
{
    if (idx->text.empty()) {
        char buf[128];
        for (const LfqFaEntry &x : idx->e) {
            idx->text += x.name;
            snprintf(buf, sizeof(buf), "\t%lld\t%lld\t%d\t%d\n", (long long)x.length, (long long)x.offset, x.line_blen, x.line_len);
            idx->text += buf;
        }
    }
    return idx->text;
}

/* .fai text -> index: name TAB length TAB offset TAB line_blen TAB line_len per line, further columns ignored; false: a line with
 * fewer fields, a field that is no non-negative decimal number or one that does not fit its type.  The first of equal names wins */
static inline bool lfq_fa_index_parse_text(const char *text, int64_t n, lfq_fasta_index *idx)
{
    idx->e.clear();
    idx->n_dup = 0;
    idx->text.clear();
    for (int64_t at = 0; at < n;) {
        int64_t eol = at;
        while (eol < n && text[eol] != '\n') {
            eol++;
        }
        int64_t f = at;
        while (f < eol && text[f] != '\t') {
            f++;
        }
        LfqFaEntry x;
        x.name.assign(text + at, (size_t)(f - at));
        int64_t v[4];
        for (int i = 0; i < 4; i++) {
            if (f >= eol || text[f] != '\t') {
                return false;
            }
            f++;
            if (f >= eol || text[f] < '0' || text[f] > '9') {
                return false;
            }
            int64_t x64 = 0;
            for (; f < eol && text[f] >= '0' && text[f] <= '9'; f++) {
                if (x64 > (INT64_MAX - 9) / 10) {
                    return false;
                }
                x64 = x64 * 10 + (text[f] - '0');
            }
            if (f < eol && text[f] != '\t' && text[f] != '\r') {
                return false;
            }
            v[i] = x64;
        }
        if (v[2] > INT32_MAX || v[3] > INT32_MAX) {
            return false;
        }
        x.length = v[0]; x.offset = v[1]; x.line_blen = (int32_t)v[2]; x.line_len = (int32_t)v[3];
        if (idx->find(x.name.c_str()) >= 0) {
            idx->n_dup++;
        } else {
            idx->e.push_back(x);
        }
        at = eol + 1;
    }
    return true;
}

/* the line starts of text[0, n): start[k] for every line and the sentinel (see the head of this file) */
static inline void lfq_fa_host_lines(const uint8_t *text, int64_t n, std::vector<int64_t> *start)
{
    start->clear();
    if (n <= 0) {
        return;
    }
    start->push_back(0);
    for (int64_t i = 0; i + 1 < n; i++) {
        if (text[i] == '\n') {
            start->push_back(i + 1);
        }
    }
    start->push_back(text[n - 1] == '\n' ? n : n + 1);
}

/* the index of text[0, n) by the rules above, one thread, line by line: what the kernels of lfq_fasta.hip compute, in the same
 * terms.  true: *idx is the index; false: *why says why not, *bad_line (1-based) and *bad_byte (-1: the file ends there) where */
static inline bool lfq_fa_host_build(const uint8_t *text, int64_t n, lfq_fasta_index *idx, int *why, int64_t *bad_line, int *bad_byte)
{
    std::vector<int64_t> st;
    lfq_fa_host_lines(text, n, &st);
    const int64_t n_lines = st.empty() ? 0 : (int64_t)st.size() - 1;
    *why = LFQ_FA_OK;
    *bad_line = 0;
    *bad_byte = 0;
    std::vector<LfqFaRaw> raw;
    std::vector<std::string> names;
    auto graph = [&](int64_t a, int64_t b) {
        int64_t g = 0;
        for (int64_t i = a; i < b && i < n; i++) {
            g += lfq_fa_isgraph(text[i]);
        }
        return g;
    };
    int64_t first = -1, m = -1;         /* of the sequence the walk is in: its first line, its first line that is not full */
    for (int64_t k = 0; k < n_lines; k++) {
        const int64_t s = st[(size_t)k], bytes = st[(size_t)k + 1] - s;
        if (text[s] == '>') {
            LfqFaRaw r;
            memset(&r, 0, sizeof(r));
            int64_t nb, nl;
            lfq_fa_name_cut(text, s + 1, std::min(st[(size_t)k + 1], n) - (st[(size_t)k + 1] <= n ? 1 : 0), &nb, &nl);
            r.name_beg = nb;
            r.name_len = (int32_t)nl;
            r.offset = st[(size_t)k + 1];
            raw.push_back(r);
            names.emplace_back((const char *)text + nb, (size_t)nl);
            first = k + 1;
            m = INT64_MAX;
            continue;
        }
        const int64_t fb = first >= 0 ? st[(size_t)first + 1] - st[(size_t)first] : 0;
        if (first >= 0 && m == INT64_MAX && !lfq_fa_line_full(bytes, fb)) {
            m = k;
        }
        const int b1 = s + 1 < n ? text[s + 1] : -1;
        const int off = lfq_fa_line_offence(k, m, bytes, fb, lfq_fa_line_skippable(bytes, text[s], b1));
        if (off != LFQ_FA_OK) {
            *why = off;
            *bad_line = k + 1;
            *bad_byte = off == LFQ_FA_UNEXPECTED && text[s] == '\r' ? b1 : text[s];
            idx->e.clear();
            return false;
        }
        if (first >= 0 && k <= m) {     /* a line of the sequence */
            LfqFaRaw &r = raw.back();
            const int64_t g = graph(s, st[(size_t)k + 1]);
            if (k == first && bytes != 1) {
                r.valid = 1;
                r.line_len = (int32_t)bytes;
                r.line_blen = (int32_t)g;
            }
            if (r.valid) {
                r.length += g;
            }
        }
    }
    *why = lfq_fa_entries_finish(raw, names, idx);
    return *why == LFQ_FA_OK;
}

/* the contig of entry x from text[0, n): true and *out, or false when offset / length do not fit the file */
static inline bool lfq_fa_host_fetch(const uint8_t *text, int64_t n, const LfqFaEntry &x, std::string *out)
{
    out->clear();
    if (x.offset < 0 || x.offset > n || x.length < 0) {
        return false;
    }
    for (int64_t i = x.offset; i < n && (int64_t)out->size() < x.length; i++) {
        if (lfq_fa_isgraph(text[i])) {
            out->push_back((char)text[i]);
        }
    }
    return (int64_t)out->size() == x.length;
}

#endif
