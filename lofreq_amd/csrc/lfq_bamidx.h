/*
 * lfq_bamidx.h -- the .bai of a BAM (lfq_bam_index_build; the rules: INTEGRATION.md section 13) for the
 * host and for the device.  lfq_bamidx.hip runs the first half with one lane per record, lfq_bamidx_check.cpp with the host compiler
 * as a stand-alone program that walks the same three passes as loops (tests/test_bai_edges.py); both call the functions below, so
 * what a record contributes is decided here.
 *
 *   record pass      lfq_bai_record(): the checks, the CIGAR's reference length, reg2bin, the virtual offsets of the record's first
 *                    byte (u) and of the byte behind it (v) by binary search in data_off, the mapped bit and the record's windows
 *   runs and chunks  record j heads a chunk when (refID, bin) differs from record j - 1's (lfq_bai_chunk_head), a reference's run
 *                    when refID does (lfq_bai_run_head); the chunk takes u from its head and v from the record in front of the next
 *                    head, the run likewise plus the positions and mapped counts at its ends
 *   linear index     the running maximum of lfq_bai_key() -- refID above the last window + 1 of a mapped record -- in front of
 *                    record j tells the windows others touched before it (lfq_bai_first_window): records are sorted, so j is the
 *                    first to touch exactly [that, its last window].  The intervals of different records never overlap, so their
 *                    order does not matter and no table per window exists before the host fills one per reference with records.
 *
 * The host half (rules 4 and 6, the file, the query) is plain C++ and is what lfq_bam_index is made of.
 */
#ifndef LFQ_BAMIDX_H
#define LFQ_BAMIDX_H

#include <stdint.h>

#if defined(__HIPCC__)
#define LFQ_BAI_FN __host__ __device__ static inline
#else
#define LFQ_BAI_FN static inline
#endif

#define LFQ_BAI_META_BIN 37450
#define LFQ_BAI_MAX_END (1 << 29)       /* BAI's limit: five levels of bins over 16 KiB windows */
#define LFQ_BAI_MIN_RECORD 36           /* block_size and the core */

/* what the record pass leaves of record j */
struct LfqBaiRec {
    uint64_t u, v;
    int32_t ref_id;                     /* < 0: no coordinates, no chunk */
    uint16_t bin, mapped;
    int32_t w0, w1;                     /* the windows [beg >> 14, (end - 1) >> 14] */
};

struct LfqBaiChunk {                    /* rule 3, in file order */
    uint64_t u, v;
    int32_t ref_id;
    uint32_t bin;
};

struct LfqBaiRun {                      /* the records of one reference (rule 5) */
    uint64_t u, v;
    int64_t first, last;                /* its first and last record */
    int64_t mapped_before, mapped_through;     /* mapped records in front of `first`, and up to and including `last` */
    int32_t ref_id, pad_;
};

struct LfqBaiIntv {                     /* the windows record `u` is the first to touch (rule 4) */
    uint64_t u;
    int32_t ref_id, w0, w1, pad_;
};

LFQ_BAI_FN int lfq_bai_reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (int)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(1 + (beg >> 26));
    return 0;
}

/* little-endian loads from bytes at any alignment */
LFQ_BAI_FN uint32_t lfq_bai_ld32(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
LFQ_BAI_FN uint32_t lfq_bai_ld16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

/* the reference bases (M D N = X) of n CIGAR words */
LFQ_BAI_FN int64_t lfq_bai_cigar_ref_len(const uint8_t *cigar, uint32_t n)
{
    int64_t len = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t w = lfq_bai_ld32(cigar + 4 * (size_t)k);
        if ((0x18du >> (w & 15u)) & 1u) {       /* ops 0 2 3 7 8 */
            len += (int64_t)(w >> 4);
        }
    }
    return len;
}

/* rule 2: the virtual offset of byte p.  The block is the last one that starts at or in front of p -- among blocks that start at the
 * same byte that is the one that is not empty --, and behind the last byte the place where the next block would start */
LFQ_BAI_FN uint64_t lfq_bai_voffset(int64_t p, const int64_t *data_off, const int64_t *comp_off, int64_t n_blocks, int64_t file_off)
{
    if (n_blocks <= 0 || p >= data_off[n_blocks]) {
        return (uint64_t)(comp_off[n_blocks > 0 ? n_blocks : 0] + file_off) << 16;
    }
    int64_t lo = 0, hi = n_blocks - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (data_off[mid] <= p) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    return ((uint64_t)(comp_off[lo] + file_off) << 16) | (uint64_t)(p - data_off[lo]);
}

/* The record pass for record j: false when the record is refused (INTEGRATION.md section 13 lists the refusals; each is decided
 * from record j and the core of record j - 1 alone, so the first bad record is the smallest j that returns false).  Reads
 * body[rec_off[j] .. rec_off[j + 1]) and eight bytes of record j - 1's core, nothing else of body. */
LFQ_BAI_FN bool lfq_bai_record(const uint8_t *body, const int64_t *rec_off, int64_t j, int32_t n_ref, const int64_t *data_off,
                               const int64_t *comp_off, int64_t n_blocks, int64_t file_off, LfqBaiRec *out)
{
    const int64_t o = rec_off[j], len = rec_off[j + 1] - o;
    const uint8_t *r = body + o;
    LfqBaiRec R;
    R.u = R.v = 0;
    R.ref_id = -1;
    R.bin = R.mapped = 0;
    R.w0 = 0;
    R.w1 = -1;
    *out = R;
    if (len < LFQ_BAI_MIN_RECORD || (int64_t)(int32_t)lfq_bai_ld32(r) + 4 != len) {
        return false;
    }
    const int32_t ref_id = (int32_t)lfq_bai_ld32(r + 4), pos = (int32_t)lfq_bai_ld32(r + 8);
    const uint32_t l_name = r[12], n_cigar = lfq_bai_ld16(r + 16), flag = lfq_bai_ld16(r + 18);
    if ((int64_t)l_name + 4 * (int64_t)n_cigar > len - LFQ_BAI_MIN_RECORD) {
        return false;
    }
    if (ref_id >= n_ref || ref_id < -1) {
        return false;
    }
    const int64_t ref_len = lfq_bai_cigar_ref_len(r + LFQ_BAI_MIN_RECORD + l_name, n_cigar);
    const bool mapped = (flag & 4u) == 0;
    const int64_t beg = pos, end = ref_len == 0 || !mapped ? beg + 1 : beg + ref_len;
    if (ref_id >= 0 && (pos < -1 || end > LFQ_BAI_MAX_END)) {
        return false;
    }
    if (j > 0 && o - rec_off[j - 1] >= LFQ_BAI_MIN_RECORD) {
        const uint8_t *q = body + rec_off[j - 1];
        const int32_t p_ref = (int32_t)lfq_bai_ld32(q + 4), p_pos = (int32_t)lfq_bai_ld32(q + 8);
        if (ref_id >= 0 && (p_ref < 0 || ref_id < p_ref || (ref_id == p_ref && pos < p_pos))) {
            return false;
        }
    }
    R.u = lfq_bai_voffset(o, data_off, comp_off, n_blocks, file_off);
    R.v = lfq_bai_voffset(o + len, data_off, comp_off, n_blocks, file_off);
    R.ref_id = ref_id;
    R.mapped = mapped ? 1 : 0;
    if (ref_id >= 0) {
        R.bin = (uint16_t)lfq_bai_reg2bin(beg, end);
        R.w0 = (int32_t)((beg > 0 ? beg : 0) >> 14);
        R.w1 = (int32_t)((end - 1) >> 14);          /* (-1 for a read at pos -1 without reference bases: it touches no window) */
    }
    *out = R;
    return true;
}

LFQ_BAI_FN bool lfq_bai_run_head(const LfqBaiRec *r, int64_t j)
{
    return r[j].ref_id >= 0 && (j == 0 || r[j - 1].ref_id != r[j].ref_id);
}
LFQ_BAI_FN bool lfq_bai_chunk_head(const LfqBaiRec *r, int64_t j)
{
    return r[j].ref_id >= 0 && (j == 0 || r[j - 1].ref_id != r[j].ref_id || r[j - 1].bin != r[j].bin);
}
/* record j is the last of its chunk / of its reference's run */
LFQ_BAI_FN bool lfq_bai_chunk_tail(const LfqBaiRec *r, int64_t j, int64_t n)
{
    return r[j].ref_id >= 0 && (j + 1 == n || r[j + 1].ref_id != r[j].ref_id || r[j + 1].bin != r[j].bin);
}
LFQ_BAI_FN bool lfq_bai_run_tail(const LfqBaiRec *r, int64_t j, int64_t n)
{
    return r[j].ref_id >= 0 && (j + 1 == n || r[j + 1].ref_id != r[j].ref_id);
}
LFQ_BAI_FN bool lfq_bai_in_linear(const LfqBaiRec &r) { return r.ref_id >= 0 && r.mapped && r.w1 >= r.w0; }

/* refID above (last window + 1): among sorted records the maximum over the records in front of j is that of j's own reference, or
 * of an earlier one, which the upper half tells */
LFQ_BAI_FN uint64_t lfq_bai_key(const LfqBaiRec &r)
{
    return lfq_bai_in_linear(r) ? ((uint64_t)(uint32_t)r.ref_id << 32) | (uint32_t)(r.w1 + 1) : 0;
}
/* the first window record r is the first to touch, given the maximum key of the records in front of it; above r.w1: none */
LFQ_BAI_FN int32_t lfq_bai_first_window(const LfqBaiRec &r, uint64_t max_before)
{
    const int32_t taken = (int32_t)(max_before >> 32) == r.ref_id ? (int32_t)(uint32_t)max_before : 0;      /* windows < taken are touched */
    return taken > r.w0 ? taken : r.w0;
}

/* ---- the host half ---------------------------------------------------------------------------------------------------------------- */
#include <string.h>

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

typedef std::pair<uint64_t, uint64_t> LfqBaiSpan;

struct LfqBaiRef {
    std::map<uint32_t, std::vector<LfqBaiSpan>> bins;   /* without the metadata pseudo-bin */
    std::vector<uint64_t> linear;
    bool has_meta = false;
    uint64_t meta[4] = {0, 0, 0, 0};    /* u of the first record, v of the last, mapped, unmapped */
};

struct lfq_bam_index {
    std::vector<LfqBaiRef> refs;
    uint64_t n_no_coor = 0;
    std::vector<uint8_t> bytes;         /* the .bai, made on first request */
    std::vector<uint64_t> q_beg, q_end; /* the last query's chunks */
};

/* the argument checks of lfq_bam_index_build that need no record */
static inline bool lfq_bai_check_args(int64_t n_bytes, const int64_t *rec_off, int64_t n_recs, const int64_t *data_off,
                                      const int64_t *comp_off, int64_t n_blocks, int64_t file_off, int32_t n_ref)
{
    if (!rec_off || !data_off || !comp_off || n_bytes < 0 || n_recs < 0 || n_blocks < 0 || n_ref < 0 || file_off < 0) {
        return false;
    }
    for (int64_t j = 0; j < n_recs; j++) {
        if (rec_off[j + 1] <= rec_off[j]) {
            return false;
        }
    }
    for (int64_t b = 0; b < n_blocks; b++) {
        if (data_off[b + 1] < data_off[b] || comp_off[b + 1] <= comp_off[b]) {
            return false;
        }
    }
    return rec_off[0] >= 0 && rec_off[n_recs] <= n_bytes && comp_off[0] >= 0 && rec_off[0] >= data_off[0]
           && rec_off[n_recs] <= data_off[n_blocks];
}

/* passes two and three as loops: what the device's compaction emits, in file order */
static inline void lfq_bai_compact_host(const LfqBaiRec *r, int64_t n, std::vector<LfqBaiChunk> *chunks, std::vector<LfqBaiRun> *runs,
                                        std::vector<LfqBaiIntv> *intvs)
{
    uint64_t max_before = 0;
    int64_t mapped = 0;
    for (int64_t j = 0; j < n; j++) {
        if (lfq_bai_chunk_head(r, j)) {
            chunks->push_back({r[j].u, 0, r[j].ref_id, r[j].bin});
        }
        if (lfq_bai_run_head(r, j)) {
            runs->push_back({r[j].u, 0, j, j, mapped, mapped, r[j].ref_id, 0});
        }
        mapped += r[j].ref_id >= 0 && r[j].mapped;
        if (lfq_bai_chunk_tail(r, j, n)) {
            chunks->back().v = r[j].v;
        }
        if (lfq_bai_run_tail(r, j, n)) {
            runs->back().v = r[j].v;
            runs->back().last = j;
            runs->back().mapped_through = mapped;
        }
        if (lfq_bai_in_linear(r[j])) {
            const int32_t w = lfq_bai_first_window(r[j], max_before);
            if (w <= r[j].w1) {
                intvs->push_back({r[j].u, r[j].ref_id, w, r[j].w1, 0});
            }
            max_before = std::max(max_before, lfq_bai_key(r[j]));
        }
    }
}

static inline int lfq_bai_bin_level(uint32_t bin)
{
    return bin >= 4681 ? 5 : bin >= 585 ? 4 : bin >= 73 ? 3 : bin >= 9 ? 2 : bin >= 1 ? 1 : 0;
}

/* rule 6 on the bins of one reference, whose chunks are in file order */
static inline void lfq_bai_merge_bins(std::map<uint32_t, std::vector<LfqBaiSpan>> *bins)
{
    for (int level = 5; level >= 1; level--) {
        std::vector<uint32_t> at_level;
        for (const auto &kv : *bins) {
            if (lfq_bai_bin_level(kv.first) == level) {
                at_level.push_back(kv.first);
            }
        }
        for (uint32_t b : at_level) {
            std::vector<LfqBaiSpan> &cs = (*bins)[b];
            std::sort(cs.begin(), cs.end());
            const auto parent = bins->find((b - 1) >> 3);
            if (parent != bins->end() && (cs.back().second >> 16) - (cs.front().first >> 16) < 65536) {
                parent->second.insert(parent->second.end(), cs.begin(), cs.end());
                bins->erase(b);
            }
        }
    }
    for (auto &kv : *bins) {
        std::vector<LfqBaiSpan> &cs = kv.second;
        std::sort(cs.begin(), cs.end());
        size_t m = 0;
        for (size_t k = 1; k < cs.size(); k++) {
            if (cs[k].first >> 16 <= cs[m].second >> 16) {
                cs[m].second = std::max(cs[m].second, cs[k].second);
            } else {
                cs[++m] = cs[k];
            }
        }
        cs.resize(m + 1);
    }
}

/* rules 3 to 6 from the compacted lists.  false: a list names a reference or a window that cannot be (the caller's LFQ_ERR_HIP) */
static inline bool lfq_bai_finish(const LfqBaiChunk *chunks, int64_t n_chunks, const LfqBaiRun *runs, int64_t n_runs,
                                  const LfqBaiIntv *intvs, int64_t n_intvs, int32_t n_ref, int64_t n_recs, lfq_bam_index *idx)
{
    idx->refs.assign((size_t)n_ref, LfqBaiRef());
    int64_t placed = 0;
    for (int64_t k = 0; k < n_chunks; k++) {
        if (chunks[k].ref_id < 0 || chunks[k].ref_id >= n_ref || chunks[k].bin >= LFQ_BAI_META_BIN) {
            return false;
        }
        idx->refs[(size_t)chunks[k].ref_id].bins[chunks[k].bin].push_back({chunks[k].u, chunks[k].v});
    }
    for (int64_t k = 0; k < n_runs; k++) {
        const LfqBaiRun &r = runs[k];
        if (r.ref_id < 0 || r.ref_id >= n_ref || r.last < r.first || idx->refs[(size_t)r.ref_id].has_meta) {
            return false;
        }
        LfqBaiRef &ref = idx->refs[(size_t)r.ref_id];
        const int64_t n = r.last - r.first + 1, mapped = r.mapped_through - r.mapped_before;
        if (mapped < 0 || mapped > n) {
            return false;
        }
        ref.has_meta = true;
        ref.meta[0] = r.u;
        ref.meta[1] = r.v;
        ref.meta[2] = (uint64_t)mapped;
        ref.meta[3] = (uint64_t)(n - mapped);
        placed += n;
    }
    if (placed > n_recs) {
        return false;
    }
    idx->n_no_coor = (uint64_t)(n_recs - placed);
    /* rule 4: n_intv per reference, then the windows each interval is the first to touch, then the fill */
    const uint64_t none = ~(uint64_t)0;
    for (int64_t k = 0; k < n_intvs; k++) {
        const LfqBaiIntv &t = intvs[k];
        if (t.ref_id < 0 || t.ref_id >= n_ref || t.w0 < 0 || t.w1 < t.w0 || t.w1 >= (LFQ_BAI_MAX_END >> 14)) {
            return false;
        }
        std::vector<uint64_t> &lin = idx->refs[(size_t)t.ref_id].linear;
        if (lin.size() < (size_t)t.w1 + 1) {
            lin.resize((size_t)t.w1 + 1, none);
        }
        for (int32_t w = t.w0; w <= t.w1; w++) {
            lin[(size_t)w] = t.u;
        }
    }
    for (LfqBaiRef &ref : idx->refs) {
        std::vector<uint64_t> &lin = ref.linear;
        size_t first = 0;
        while (first < lin.size() && lin[first] == none) {
            first++;
        }
        for (size_t w = 0; w < lin.size(); w++) {
            if (lin[w] == none) {
                lin[w] = w < first ? lin[first] : lin[w - 1];
            }
        }
        lfq_bai_merge_bins(&ref.bins);
    }
    return true;
}

/* rule 7 */
static inline void lfq_bai_put(std::vector<uint8_t> *out, uint64_t v, int bytes)
{
    for (int k = 0; k < bytes; k++) {
        out->push_back((uint8_t)(v >> (8 * k)));
    }
}

static inline void lfq_bai_serialise(const lfq_bam_index &idx, std::vector<uint8_t> *out)
{
    out->clear();
    for (char c : {'B', 'A', 'I', '\1'}) {
        out->push_back((uint8_t)c);
    }
    lfq_bai_put(out, idx.refs.size(), 4);
    for (const LfqBaiRef &ref : idx.refs) {
        lfq_bai_put(out, ref.bins.size() + (ref.has_meta ? 1 : 0), 4);
        for (const auto &kv : ref.bins) {
            lfq_bai_put(out, kv.first, 4);
            lfq_bai_put(out, kv.second.size(), 4);
            for (const LfqBaiSpan &c : kv.second) {
                lfq_bai_put(out, c.first, 8);
                lfq_bai_put(out, c.second, 8);
            }
        }
        if (ref.has_meta) {
            lfq_bai_put(out, LFQ_BAI_META_BIN, 4);
            lfq_bai_put(out, 2, 4);
            for (uint64_t v : ref.meta) {
                lfq_bai_put(out, v, 8);
            }
        }
        lfq_bai_put(out, ref.linear.size(), 4);
        for (uint64_t v : ref.linear) {
            lfq_bai_put(out, v, 8);
        }
    }
    lfq_bai_put(out, idx.n_no_coor, 8);
}

static inline uint64_t lfq_bai_get(const uint8_t *p, int bytes)
{
    uint64_t v = 0;
    for (int k = 0; k < bytes; k++) {
        v |= (uint64_t)p[k] << (8 * k);
    }
    return v;
}

/* a .bai as any writer lays it out: bins in any order, the trailing n_no_coor optional.  false: not a .bai -- a count that runs past
 * the file, a bin twice, a metadata bin without exactly two chunks, bytes left over */
static inline bool lfq_bai_parse(const uint8_t *bai, int64_t n_bytes, lfq_bam_index *idx)
{
    if (n_bytes < 8 || memcmp(bai, "BAI\1", 4) != 0) {
        return false;
    }
    const int64_t n_ref = (int32_t)lfq_bai_get(bai + 4, 4);
    int64_t o = 8;
    if (n_ref < 0 || n_ref > (n_bytes - 8) / 8) {       /* (eight bytes a reference at least) */
        return false;
    }
    idx->refs.assign((size_t)n_ref, LfqBaiRef());
    for (LfqBaiRef &ref : idx->refs) {
        if (o + 4 > n_bytes) {
            return false;
        }
        const int64_t n_bin = (int32_t)lfq_bai_get(bai + o, 4);
        o += 4;
        if (n_bin < 0) {
            return false;
        }
        for (int64_t b = 0; b < n_bin; b++) {
            if (o + 8 > n_bytes) {
                return false;
            }
            const uint32_t bin = (uint32_t)lfq_bai_get(bai + o, 4);
            const int64_t n_chunk = (int32_t)lfq_bai_get(bai + o + 4, 4);
            o += 8;
            if (n_chunk < 0 || n_chunk > (n_bytes - o) / 16) {
                return false;
            }
            if (bin == LFQ_BAI_META_BIN) {
                if (n_chunk != 2 || ref.has_meta) {
                    return false;
                }
                ref.has_meta = true;
                for (int k = 0; k < 4; k++) {
                    ref.meta[k] = lfq_bai_get(bai + o + 8 * k, 8);
                }
            } else {
                if (bin > LFQ_BAI_META_BIN || ref.bins.count(bin)) {
                    return false;
                }
                std::vector<LfqBaiSpan> &cs = ref.bins[bin];
                for (int64_t k = 0; k < n_chunk; k++) {
                    cs.push_back({lfq_bai_get(bai + o + 16 * k, 8), lfq_bai_get(bai + o + 16 * k + 8, 8)});
                }
            }
            o += 16 * n_chunk;
        }
        if (o + 4 > n_bytes) {
            return false;
        }
        const int64_t n_intv = (int32_t)lfq_bai_get(bai + o, 4);
        o += 4;
        if (n_intv < 0 || n_intv > (n_bytes - o) / 8) {
            return false;
        }
        for (int64_t k = 0; k < n_intv; k++) {
            ref.linear.push_back(lfq_bai_get(bai + o + 8 * k, 8));
        }
        o += 8 * n_intv;
    }
    idx->n_no_coor = 0;
    if (o + 8 <= n_bytes) {
        idx->n_no_coor = lfq_bai_get(bai + o, 8);
        o += 8;
    }
    return o == n_bytes;
}

/* the bins that may hold a record overlapping [beg, end), 0 <= beg < end <= 2^29 */
static inline void lfq_bai_reg2bins(int64_t beg, int64_t end, std::vector<uint32_t> *bins)
{
    --end;
    bins->assign(1, 0);
    static const int shift[5] = {26, 23, 20, 17, 14}, base[5] = {1, 9, 73, 585, 4681};
    for (int l = 0; l < 5; l++) {
        for (int64_t k = base[l] + (beg >> shift[l]); k <= base[l] + (end >> shift[l]); k++) {
            bins->push_back((uint32_t)k);
        }
    }
}

/* lfq_bam_index_query: the chunks of those bins that end above the linear index's value for beg >> 14 (0 past n_intv), begun no
 * earlier than that value, sorted, overlapping or touching ones merged */
static inline void lfq_bai_query(lfq_bam_index *idx, int32_t tid, int64_t beg, int64_t end)
{
    idx->q_beg.clear();
    idx->q_end.clear();
    if (tid < 0 || (size_t)tid >= idx->refs.size() || end <= beg || end <= 0) {
        return;
    }
    beg = std::max<int64_t>(beg, 0);
    end = std::min<int64_t>(end, LFQ_BAI_MAX_END);
    if (beg >= end) {
        return;
    }
    const LfqBaiRef &ref = idx->refs[(size_t)tid];
    const size_t w = (size_t)(beg >> 14);
    const uint64_t min_off = w < ref.linear.size() ? ref.linear[w] : 0;
    std::vector<uint32_t> bins;
    lfq_bai_reg2bins(beg, end, &bins);
    std::vector<LfqBaiSpan> cs;
    for (uint32_t b : bins) {
        const auto it = ref.bins.find(b);
        if (it == ref.bins.end()) {
            continue;
        }
        for (const LfqBaiSpan &c : it->second) {
            if (c.second > min_off) {
                cs.push_back({std::max(c.first, min_off), c.second});
            }
        }
    }
    std::sort(cs.begin(), cs.end());
    for (const LfqBaiSpan &c : cs) {
        if (!idx->q_beg.empty() && c.first <= idx->q_end.back()) {
            idx->q_end.back() = std::max(idx->q_end.back(), c.second);
        } else {
            idx->q_beg.push_back(c.first);
            idx->q_end.push_back(c.second);
        }
    }
}

#endif
