/*
 * lfq_bed.h -- the targets of `lofreq call -l` (lfq_set_bed; the rules: INTEGRATION.md section 9) for the
 * host and for the device: the table of one name, the overlap predicate both sides compile, and the parser (host only).
 * lfq_bed.hip applies the predicate with one lane per read and one per position; lfq_bed_check.cpp is the header's stand-alone
 * program for the host compiler (tests/test_bed_edges.py).
 *
 *   table      per name the intervals sorted by (beg, end) as bedidx.c's ks_introsort leaves them: beg[], end[], and pmax[k] = the
 *              largest end of the intervals 0 .. k.  Duplicates, overlaps and zero-length intervals stay as they are: [x, x)
 *              matches a read with pos < x < endpos and no column, which a union of the intervals would lose.
 *   predicate  [beg, end) overlaps iff some interval has end_i > beg and beg_i < end (bed_overlap_core's test; its 8 kb linear
 *              index only chooses where the scan starts).  The intervals with beg_i < end are the first k of the sorted table, so
 *              the answer is pmax[k - 1] > beg: one binary search and one load.
 *   parser     bed_read (bedidx.c:159-244), line by line; what it refuses is refused here, plus any value above INT32_MAX, which
 *              the reference compares as a negative int.
 */
#ifndef LFQ_BED_H
#define LFQ_BED_H

#include <stdint.h>

#if defined(__HIPCC__)
#define LFQ_BED_FN __host__ __device__ static inline
#else
#define LFQ_BED_FN static inline
#endif

/* the table of one name as the kernels take it (device pointers there, host pointers in lfq_bed_overlap); n = 0: nothing overlaps */
struct LfqBedTab {
    const int32_t *beg;                 /* [n] ascending */
    const int32_t *pmax;                /* [n] running maximum of the ends in that order */
    int64_t n;
};

LFQ_BED_FN int lfq_bed_tab_overlap(const LfqBedTab &t, int64_t beg, int64_t end)
{
    int64_t lo = 0, hi = t.n;           /* -> the number of intervals with beg_i < end */
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)t.beg[mid] < end) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return lo > 0 && (int64_t)t.pmax[lo - 1] > beg;
}

/* bam_endpos from n CIGAR words: pos + the reference bases of M D N = X, pos + 1 when there are none */
LFQ_BED_FN int64_t lfq_bed_endpos(int64_t pos, const uint32_t *cigar, int64_t n)
{
    int64_t rlen = 0;
    for (int64_t k = 0; k < n; k++) {
        const uint32_t op = cigar[k] & 0xfu;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) {
            rlen += cigar[k] >> 4;
        }
    }
    return pos + (rlen > 0 ? rlen : 1);
}

/* ---- host only from here on ---- */
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

struct LfqBedName {
    std::string name;
    std::vector<int32_t> beg, end, pmax;
    LfqBedTab tab() const { return {beg.data(), pmax.data(), (int64_t)beg.size()}; }
};

struct lfq_bed {
    std::vector<LfqBedName> names;      /* in order of first appearance */
    const LfqBedName *find(const char *name) const
    {
        for (const LfqBedName &t : names) {
            if (name && t.name == name) {
                return &t;
            }
        }
        return nullptr;
    }
};

static inline bool lfq_bed_isspace(char ch)     /* isspace() of the C locale */
{
    return ch == ' ' || ch == '\t' || ch == '\n' || ch == '\v' || ch == '\f' || ch == '\r';
}

/* sscanf's %u at s: blanks, a sign, decimal digits -> the value as the reference's unsigned int holds it, saturated above 32 bits
 * (1 << 32: "too large" whatever follows); false: no number.  *s moves behind what was read */
static inline bool lfq_bed_scan_u(const char *&s, const char *e, uint64_t *v)
{
    while (s < e && lfq_bed_isspace(*s)) {
        s++;
    }
    bool neg = false;
    if (s < e && (*s == '+' || *s == '-')) {
        neg = *s == '-';
        s++;
    }
    if (s >= e || *s < '0' || *s > '9') {
        return false;
    }
    uint64_t x = 0;
    for (; s < e && *s >= '0' && *s <= '9'; s++) {
        x = x * 10 + (uint64_t)(*s - '0');
        if (x > ((uint64_t)1 << 32)) {
            x = (uint64_t)1 << 32;
        }
    }
    *v = (neg && x != 0) ? ((uint64_t)1 << 32) : x;     /* -5 is 4294967291 to the reference: above every end either way */
    return true;
}

/* text[0 .. n) -> *bed.  true: parsed (an empty line ends the text, as the reference's read loop does); false: line *bad_line
 * (1-based) is refused and *bed is empty */
static inline bool lfq_bed_parse_text(const char *text, int64_t n, lfq_bed *bed, int64_t *bad_line)
{
    bed->names.clear();
    std::vector<std::vector<std::pair<int32_t, int32_t>>> iv;
    int64_t line = 0;
    for (int64_t at = 0; at < n;) {
        int64_t eol = at;
        while (eol < n && text[eol] != '\n') {
            eol++;
        }
        if (eol == at) {
            break;                                          /* ks_getuntil returns 0: the loop ends, silently */
        }
        line++;
        const char *s = text + at, *e = text + eol;
        at = eol + 1;
        const char *nul = (const char *)memchr(s, 0, (size_t)(e - s));
        if (nul) {
            e = nul;                                        /* the line is a C string to the reference */
        }
        while (s < e && lfq_bed_isspace(*s)) {
            s++;
        }
        if (s == e || *s == '#') {
            continue;
        }
        const char *name_end = s;
        while (name_end < e && !lfq_bed_isspace(*name_end)) {
            name_end++;
        }
        const std::string name(s, name_end);
        int num = 0;
        uint64_t beg = 0, end = 0;
        if (name_end < e) {
            const char *q = name_end + 1;
            if (lfq_bed_scan_u(q, e, &beg)) {
                num = lfq_bed_scan_u(q, e, &end) ? 2 : 1;
            }
        }
        if (num == 1) {                                     /* the position list: 1-based */
            end = beg;
            beg = beg == 0 ? ((uint64_t)1 << 32) : beg - 1; /* (0 wraps to UINT_MAX there: end < beg) */
        }
        if (num < 1 || end < beg || beg > (uint64_t)INT32_MAX || end > (uint64_t)INT32_MAX) {
            if (name == "browser" || name == "track") {
                continue;
            }
            bed->names.clear();
            if (bad_line) {
                *bad_line = line;
            }
            return false;
        }
        size_t t = 0;
        while (t < bed->names.size() && bed->names[t].name != name) {
            t++;
        }
        if (t == bed->names.size()) {
            bed->names.emplace_back();
            bed->names.back().name = name;
            iv.emplace_back();
        }
        iv[t].push_back({(int32_t)beg, (int32_t)end});
    }
    for (size_t t = 0; t < iv.size(); t++) {
        std::sort(iv[t].begin(), iv[t].end());
        LfqBedName &T = bed->names[t];
        int32_t run = INT32_MIN;
        for (const auto &p : iv[t]) {
            run = std::max(run, p.second);
            T.beg.push_back(p.first);
            T.end.push_back(p.second);
            T.pmax.push_back(run);
        }
    }
    return true;
}

#endif
