/*
 * lfq_tbx.h -- the .tbi of a bgzipped VCF (lfq_vcf_index_*; the rules: INTEGRATION.md section 14) for the
 * host and for the device, over lfq_vcf.h (what a line is) and lfq_bamidx.h (what an htslib index of min_shift 14 and five levels is:
 * a .tbi and a .bai differ by a header and a name table).  lfq_tbx.hip runs the record pass with a lane per record of an open
 * tabix-mode file, lfq_tbx_check.cpp with the host compiler as a stand-alone program (tests/test_tbi_edges.py); both call the
 * functions below.  Each rule is held to the 2.1.4 binary's own files by tests/golden/tbi_binary.json.
 *
 *   interval   of tabix-mode record r (tbx_parse1's VCF branch): beg = POS - 1; end = the value of INFO's END= where
 *              lfq_vc_interval_ok's own finder finds one with a value, else beg + len(REF) (lfq_tbx_interval).
 *   range      hts_idx_check_range: a .tbi holds beg <= 2^29 and end <= 2^29; as end > beg, end > 2^29 is what refuses.  POS 2^29 is
 *              taken, POS 2^29 + 1 and END=2^29 + 1 are LFQ_VCF_RANGE.  An END= of more than 18 digits cannot be read and is refused
 *              the same way.  (The binary then writes no index, warns and exits with status 0.)
 *   record     refID = the CHROM run's number (names in order of first appearance), bin = reg2bin(beg, end), mapped = 1, the windows
 *              [beg >> 14, (end - 1) >> 14].
 *   offsets    htslib pushes a record with the offset BEHIND it and takes the chunk's begin from the offset it kept of the push before
 *              (hts_idx_push: last_off), so
 *                u of record 0      the virtual offset of its own line's first byte: behind every '#' line in front of it
 *                u of record r > 0  v of record r - 1.  Without a '#' line between them that is the line's own first byte; with '#'
 *                                   lines between two records -- inside a run or between runs -- it is the first of THOSE lines
 *                v of record r      the offset behind its '\n'; of the LAST record the text's end (hts_idx_finish's final offset),
 *                                   which lies behind any '#' line that follows it: where the end-of-file marker starts (empty
 *                                   blocks at the tables' end are dropped, lfq_tbx_trim_blocks).
 *              Seen in the binary's .tbi of a file with a `#`-CHROM record behind the header, between the records of a run, between
 *              two runs and at the end (`filter` writes such records through and tbx_index_build then skips them as meta lines: the
 *              rows hash_* of tests/tbi_edges.py).  Chunks therefore begin and end on line boundaries, and every record's line
 *              starts inside [u, v).
 *   container  "TBI\1", n_ref, format 2, col_seq 1, col_beg 2, col_end 0, meta '#', skip 0, l_nm, the names NUL-terminated, then
 *              what lfq_bai_serialise writes behind a .bai's n_ref, n_no_coor (0) included.  A parsed file's six settings are kept.
 */
#ifndef LFQ_TBX_H
#define LFQ_TBX_H

#include <string>

#include "lfq_vcf.h"
#include "lfq_bamidx.h"

#define LFQ_VC_RANGE 8              /* include/lofreq_amd.h: LFQ_VCF_RANGE.  Only lfq_vcf_index_build reports it, with a word of its own */
#define LFQ_TBX_MAX_END LFQ_BAI_MAX_END

/* the interval of the record on line k; false: LFQ_VC_RANGE.  The line has passed lfq_vc_interval_ok (the open refuses the others) */
LFQ_FA_FN bool lfq_tbx_interval(const LfqVcTab &T, int64_t k, int64_t *beg, int64_t *end)
{
    const uint16_t *off = T.off + k * LFQ_VC_NOFF;
    *beg = T.pos[k];
    *end = *beg + (lfq_vc_fend(off, 3) - lfq_vc_fbeg(off, 3));
    int64_t b, e, vb, ve;
    if (lfq_vc_info_range(T, k, &b, &e) && lfq_vc_info_key(T.text, b, e, "END", 3, &vb, &ve) && vb >= 0) {
        bool many = false;
        *end = lfq_vc_atol(T.text, vb, ve, 18, &many);
        if (many) {
            return false;
        }
    }
    return *beg >= 0 && *end > *beg && *end <= LFQ_TBX_MAX_END;
}

/* where line k ends: behind its '\n', or the text's end */
LFQ_FA_FN int64_t lfq_tbx_line_end(const LfqVcTab &T, int64_t k) { return T.lstart[k + 1] < T.n ? T.lstart[k + 1] : T.n; }

/* the record pass for record r of a tabix-mode file; false: LFQ_VC_RANGE (its line is lfq_vc_line_of(T, r)).  Reads the table and,
 * where INFO has an END key, that field of the text */
LFQ_FA_FN bool lfq_tbx_record(const LfqVcTab &T, int64_t r, const int64_t *data_off, const int64_t *comp_off, int64_t n_blocks,
                              int64_t file_off, LfqBaiRec *out)
{
    const int64_t k = lfq_vc_line_of(T, r);
    LfqBaiRec R;
    R.u = R.v = 0;
    R.ref_id = -1;
    R.bin = R.mapped = 0;
    R.w0 = 0;
    R.w1 = -1;
    *out = R;
    int64_t beg, end;
    if (!lfq_tbx_interval(T, k, &beg, &end)) {
        return false;
    }
    const int64_t from = r > 0 ? lfq_tbx_line_end(T, lfq_vc_line_of(T, r - 1)) : T.lstart[k];
    const int64_t to = r + 1 == T.n_rec ? T.n : lfq_tbx_line_end(T, k);
    R.u = lfq_bai_voffset(from, data_off, comp_off, n_blocks, file_off);
    R.v = lfq_bai_voffset(to, data_off, comp_off, n_blocks, file_off);
    R.ref_id = T.run_id[r];
    R.mapped = 1;
    R.bin = (uint16_t)lfq_bai_reg2bin(beg, end);
    R.w0 = (int32_t)(beg >> 14);
    R.w1 = (int32_t)((end - 1) >> 14);
    *out = R;
    return true;
}

/* ---- the host half ---------------------------------------------------------------------------------------------------------------- */
struct lfq_vcf_index {
    lfq_bam_index body;                 /* refs[i] belongs to names[i]; its q_beg / q_end hold the last query's chunks */
    std::vector<std::string> names;
    int32_t conf[6] = {2, 1, 2, 0, '#', 0};     /* format, col_seq, col_beg, col_end, meta, skip */
    std::vector<uint8_t> bytes;         /* the .tbi, made on first request */
};

/* the argument checks of lfq_vcf_index_build that need no device */
static inline bool lfq_tbx_check_args(int64_t n_text, const int64_t *data_off, const int64_t *comp_off, int64_t n_blocks, int64_t file_off)
{
    if (!data_off || !comp_off || n_text < 0 || n_blocks < 0 || file_off < 0 || comp_off[0] < 0 || data_off[0] != 0) {
        return false;
    }
    for (int64_t b = 0; b < n_blocks; b++) {
        if (data_off[b + 1] < data_off[b] || comp_off[b + 1] <= comp_off[b]) {
            return false;
        }
    }
    return data_off[n_blocks] == n_text;
}

/* the blocks without the empty ones at the tables' end -- the end-of-file marker, which an lfq_bgzf_result lists and an
 * lfq_bgzf_deflated does not --, so that the text's end is where the marker starts, as in the binary's files */
static inline int64_t lfq_tbx_trim_blocks(const int64_t *data_off, int64_t n_blocks)
{
    while (n_blocks > 0 && data_off[n_blocks] == data_off[n_blocks - 1]) {
        n_blocks--;
    }
    return n_blocks;
}

static inline void lfq_tbx_serialise(const lfq_vcf_index &idx, std::vector<uint8_t> *out)
{
    out->clear();
    for (char c : {'T', 'B', 'I', '\1'}) {
        out->push_back((uint8_t)c);
    }
    lfq_bai_put(out, idx.names.size(), 4);
    for (int32_t v : idx.conf) {
        lfq_bai_put(out, (uint32_t)v, 4);
    }
    size_t l_nm = 0;
    for (const std::string &s : idx.names) {
        l_nm += s.size() + 1;
    }
    lfq_bai_put(out, l_nm, 4);
    for (const std::string &s : idx.names) {
        out->insert(out->end(), s.begin(), s.end());
        out->push_back(0);
    }
    std::vector<uint8_t> bai;
    lfq_bai_serialise(idx.body, &bai);
    out->insert(out->end(), bai.begin() + 8, bai.end());       /* (behind "BAI\1" and n_ref) */
}

/* a .tbi as any writer lays it out, inflated.  false: no magic, a count past the end, l_nm that is not exactly n_ref NUL-terminated
 * names, a name twice, and what lfq_bai_parse refuses of the rest */
static inline bool lfq_tbx_parse(const uint8_t *tbi, int64_t n_bytes, lfq_vcf_index *idx)
{
    if (n_bytes < 36 || memcmp(tbi, "TBI\1", 4) != 0) {
        return false;
    }
    const int64_t n_ref = (int32_t)lfq_bai_get(tbi + 4, 4), l_nm = (int32_t)lfq_bai_get(tbi + 32, 4);
    if (n_ref < 0 || l_nm < 0 || l_nm > n_bytes - 36 || n_ref > l_nm) {
        return false;
    }
    for (int k = 0; k < 6; k++) {
        idx->conf[k] = (int32_t)lfq_bai_get(tbi + 8 + 4 * k, 4);
    }
    idx->names.clear();
    for (int64_t o = 0; o < l_nm;) {
        const void *z = memchr(tbi + 36 + o, 0, (size_t)(l_nm - o));
        if (!z || (int64_t)idx->names.size() == n_ref) {
            return false;
        }
        const int64_t len = (const uint8_t *)z - (tbi + 36 + o);
        idx->names.emplace_back((const char *)tbi + 36 + o, (size_t)len);
        o += len + 1;
    }
    if ((int64_t)idx->names.size() != n_ref) {
        return false;
    }
    std::vector<std::string> sorted = idx->names;
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
        return false;
    }
    std::vector<uint8_t> bai;
    for (char c : {'B', 'A', 'I', '\1'}) {
        bai.push_back((uint8_t)c);
    }
    lfq_bai_put(&bai, (uint64_t)n_ref, 4);
    bai.insert(bai.end(), tbi + 36 + l_nm, tbi + n_bytes);
    return lfq_bai_parse(bai.data(), (int64_t)bai.size(), &idx->body);
}

/* the name's number, -1: the index has no such name */
static inline int32_t lfq_tbx_name_id(const lfq_vcf_index &idx, const char *chrom)
{
    for (size_t i = 0; i < idx.names.size(); i++) {
        if (idx.names[i] == chrom) {
            return (int32_t)i;
        }
    }
    return -1;
}

/* lfq_vcf_index_query: by name, then lfq_bai_query; a name the index lacks has no chunks */
static inline void lfq_tbx_query(lfq_vcf_index *idx, const char *chrom, int64_t beg, int64_t end)
{
    lfq_bai_query(&idx->body, lfq_tbx_name_id(*idx, chrom), beg, end);
}

/* the record pass and the compaction as loops over an opened host file, then lfq_bai_finish: what lfq_vcf_index_build computes.
 * -> LFQ_VC_OK, or LFQ_VC_RANGE with the 1-based first bad line */
static inline int lfq_tbx_host_build(const LfqVcHostFile &F, const int64_t *data_off, const int64_t *comp_off, int64_t n_blocks,
                                     int64_t file_off, lfq_vcf_index *idx, int64_t *bad_line)
{
    const LfqVcTab T = F.tab();
    *bad_line = 0;
    *idx = lfq_vcf_index();
    std::vector<LfqBaiRec> recs((size_t)F.n_rec);
    int64_t bad = -1;
    for (int64_t r = F.n_rec - 1; r >= 0; r--) {        /* any order: the smallest refused line is kept */
        if (!lfq_tbx_record(T, r, data_off, comp_off, n_blocks, file_off, &recs[(size_t)r])) {
            bad = lfq_vc_line_of(T, r);
        }
    }
    if (bad >= 0) {
        *bad_line = bad + 1;
        return LFQ_VC_RANGE;
    }
    std::vector<LfqBaiChunk> chunks;
    std::vector<LfqBaiRun> runs;
    std::vector<LfqBaiIntv> intvs;
    lfq_bai_compact_host(recs.data(), F.n_rec, &chunks, &runs, &intvs);
    idx->names = F.run_name;
    if (!lfq_bai_finish(chunks.data(), (int64_t)chunks.size(), runs.data(), (int64_t)runs.size(), intvs.data(), (int64_t)intvs.size(),
                        (int32_t)F.run_name.size(), F.n_rec, &idx->body)) {
        return -1;
    }
    return LFQ_VC_OK;
}

#endif
