/*
 * lfq_tbx.hip -- the .tbi of a bgzipped VCF built on the device (lfq_vcf_index_build) and a region opened
 * through one (lfq_vcf_open_indexed), over lfq_tbx.h, which says what a record contributes.
 *
 *   lfq_tbx_record_kernel   one lane per record of an open tabix-mode lfq_vcf: lfq_tbx_record() from the table the open left on the
 *                           device (line starts, POS, REF's bounds, the CHROM run) into an LfqBaiRec; the text is read only where
 *                           INFO has an END key.  The first line the index cannot hold by an atomic minimum on one word, which the
 *                           host reads before anything else is launched.
 *   then lfq_bamidx.hip's lfq_bai_part_kernel / _scan_kernel / _emit_kernel as they are (lfq_bai_reserve, lfq_bai_compact), and
 *   lfq_bai_finish on the host.
 *
 * Device memory: the two block tables and lfq_bamidx.hip's buffers, O(records + blocks); four launches whatever the record count.
 * Host only, below the build: lfq_vcf_index_bytes / _parse / _n_names / _name / _query / _free.
 */
#include <chrono>

#include "lfq_ctx.h"
#include "lfq_tbx.h"

#define LFQ_TBX_THREADS 256

struct LfqTbxArgs {
    LfqVcTab T;                         /* the open file's table, on the device */
    const int64_t *data_off, *comp_off; /* [n_blocks + 1] */
    int64_t n_blocks, file_off;
    LfqBaiRec *rec;                     /* [T.n_rec] */
    unsigned long long *counters;       /* 0: the first line refused */
};

__global__ __launch_bounds__(LFQ_TBX_THREADS) void lfq_tbx_record_kernel(LfqTbxArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * LFQ_TBX_THREADS + threadIdx.x;
    if (r >= A.T.n_rec) {
        return;
    }
    LfqBaiRec R;
    if (!lfq_tbx_record(A.T, r, A.data_off, A.comp_off, A.n_blocks, A.file_off, &R)) {
        atomicMin(&A.counters[0], (unsigned long long)lfq_vc_line_of(A.T, r));
    }
    A.rec[r] = R;
}

static int tbx_ms(const LfqEvPair &t, double *acc)
{
    double ms = 0.0;
    LFQ_TRY(t.ms(&ms));
    *acc += ms;
    return LFQ_OK;
}

/* BSIZE of the BGZF block at comp[p ..), 0: no block header stands there */
static int64_t tbx_block_size(const uint8_t *comp, int64_t n, int64_t p)
{
    if (p < 0 || n - p < 18 || comp[p] != 31 || comp[p + 1] != 139 || comp[p + 2] != 8 || !(comp[p + 3] & 4)) {
        return 0;
    }
    const int64_t xlen = (int64_t)comp[p + 10] | ((int64_t)comp[p + 11] << 8);
    if (p + 12 + xlen > n) {
        return 0;
    }
    for (int64_t q = p + 12; q + 4 <= p + 12 + xlen;) {
        const int64_t slen = (int64_t)comp[q + 2] | ((int64_t)comp[q + 3] << 8);
        if (comp[q] == 'B' && comp[q + 1] == 'C' && slen == 2 && q + 6 <= p + 12 + xlen) {
            const int64_t size = ((int64_t)comp[q + 4] | ((int64_t)comp[q + 5] << 8)) + 1;
            return p + size <= n ? size : 0;
        }
        q += 4 + slen;
    }
    return 0;
}

extern "C" {

int lfq_vcf_index_build(lfq_vcf *v, const int64_t *data_off, const int64_t *comp_off, int64_t n_blocks, int64_t file_off,
                        lfq_vcf_index **out, int *why_out, int64_t *bad_line_out)
{
    if (out) *out = nullptr;
    if (why_out) *why_out = LFQ_VC_OK;
    if (bad_line_out) *bad_line_out = 0;
    if (!v || !out) {
        return LFQ_ERR_INVALID;
    }
    lfq_ctx *c = nullptr;
    int mode = LFQ_VC_STREAM;
    LfqVcTab T;
    const std::vector<std::string> *names = nullptr;
    lfq_vcf_view(v, &c, &mode, &T, &names);
    lfq_vcf_index_times *times = lfq_bai_vcf_times(c);
    memset(times, 0, sizeof(*times));
    if (mode != LFQ_VC_TABIX || !lfq_tbx_check_args(T.n, data_off, comp_off, n_blocks, file_off)) {
        return LFQ_ERR_INVALID;
    }
    n_blocks = lfq_tbx_trim_blocks(data_off, n_blocks);
    const int64_t nr = T.n_rec;
    if (nr > INT32_MAX) {
        return LFQ_ERR_CAPACITY;
    }
    times->n_records = nr;
    lfq_vcf_index *idx = new lfq_vcf_index();
    if (nr == 0) {
        *out = idx;
        return LFQ_OK;
    }
    struct Drop {                       /* the index is the caller's only when the call succeeds */
        lfq_vcf_index *p;
        ~Drop() { delete p; }
    } drop = {idx};
    LFQ_TRY_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t o_coff = lfq_al((n_blocks + 1) * 8), head = o_coff + lfq_al((n_blocks + 1) * 8);
    LfqBaiDev dev;
    LFQ_TRY(lfq_bai_reserve(c, head, nr, T.n_runs, &dev));
    LfqPin<int64_t> tab(c, (size_t)(2 * (n_blocks + 1)));
    LFQ_PIN_OK(tab);
    LfqPin<unsigned long long> cnt(c, 4);
    LFQ_PIN_OK(cnt);
    memcpy(tab.data(), data_off, (size_t)(n_blocks + 1) * 8);
    memcpy(tab.data() + n_blocks + 1, comp_off, (size_t)(n_blocks + 1) * 8);
    cnt[0] = ~0ull;
    cnt[1] = cnt[2] = cnt[3] = 0;
    LFQ_TRY_HIP(hipMemcpyAsync(dev.head, tab.data(), (size_t)(n_blocks + 1) * 8, hipMemcpyHostToDevice, st));
    LFQ_TRY_HIP(hipMemcpyAsync(dev.head + o_coff, tab.data() + n_blocks + 1, (size_t)(n_blocks + 1) * 8, hipMemcpyHostToDevice, st));
    LFQ_TRY_HIP(hipMemcpyAsync(dev.counters, cnt.data(), 32, hipMemcpyHostToDevice, st));
    LfqTbxArgs A;
    A.T = T;
    A.data_off = (const int64_t *)dev.head;
    A.comp_off = (const int64_t *)(dev.head + o_coff);
    A.n_blocks = n_blocks;
    A.file_off = file_off;
    A.rec = dev.rec;
    A.counters = dev.counters;
    LfqEvPair kern_t = {};
    struct DropEv {
        LfqEvPair *t;
        ~DropEv() { t->destroy(); }
    } drop_ev = {&kern_t};
    LFQ_TRY(kern_t.begin(st));
    hipLaunchKernelGGL(lfq_tbx_record_kernel, dim3((unsigned)((nr + LFQ_TBX_THREADS - 1) / LFQ_TBX_THREADS)), dim3(LFQ_TBX_THREADS), 0,
                       st, A);
    LFQ_TRY_HIP(hipGetLastError());
    LFQ_TRY(kern_t.end(st));
    times->n_launches = 1;
    /* the first refused line, before the lists are made */
    LFQ_TRY_HIP(hipMemcpyAsync(cnt.data(), dev.counters, 8, hipMemcpyDeviceToHost, st));
    LFQ_TRY_HIP(hipStreamSynchronize(st));
    LFQ_TRY(tbx_ms(kern_t, &times->kernels_ms));
    if (cnt[0] != ~0ull) {
        if (why_out) *why_out = LFQ_VC_RANGE;
        if (bad_line_out) *bad_line_out = (int64_t)cnt[0] + 1;
        return LFQ_ERR_INVALID;
    }
    LfqBaiLists L;
    LFQ_TRY(lfq_bai_compact(c, &L));
    times->n_launches = 4;
    times->kernels_ms += L.kernels_ms;
    times->download_ms += L.download_ms;
    times->n_chunks = L.n_chunks;
    times->n_intervals = L.n_intvs;
    const auto t0 = std::chrono::steady_clock::now();
    idx->names = *names;
    if (!lfq_bai_finish(L.chunks, L.n_chunks, L.runs, L.n_runs, L.intvs, L.n_intvs, (int32_t)names->size(), nr, &idx->body)) {
        return LFQ_ERR_HIP;
    }
    times->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    drop.p = nullptr;
    *out = idx;
    return LFQ_OK;
}

int lfq_last_vcf_index_times(lfq_ctx *c, lfq_vcf_index_times *t)
{
    if (!c || !t) {
        return LFQ_ERR_INVALID;
    }
    *t = *lfq_bai_vcf_times(c);
    return LFQ_OK;
}

/* ---- host only: no context ---------------------------------------------------------------------------------------------------------- */
int lfq_vcf_index_bytes(const lfq_vcf_index *idx, const uint8_t **tbi, int64_t *n_bytes)
{
    if (!idx || !tbi || !n_bytes) {
        return LFQ_ERR_INVALID;
    }
    lfq_vcf_index *m = const_cast<lfq_vcf_index *>(idx);        /* (the cache of the serialised form is not part of its value) */
    if (m->bytes.empty()) {
        lfq_tbx_serialise(*m, &m->bytes);
    }
    *tbi = m->bytes.data();
    *n_bytes = (int64_t)m->bytes.size();
    return LFQ_OK;
}

int lfq_vcf_index_parse(const uint8_t *tbi, int64_t n_bytes, lfq_vcf_index **out)
{
    if (out) *out = nullptr;
    if (!tbi || !out || n_bytes < 0) {
        return LFQ_ERR_INVALID;
    }
    lfq_vcf_index *idx = new lfq_vcf_index();
    if (!lfq_tbx_parse(tbi, n_bytes, idx)) {
        delete idx;
        return LFQ_ERR_INVALID;
    }
    *out = idx;
    return LFQ_OK;
}

int64_t lfq_vcf_index_n_names(const lfq_vcf_index *idx) { return idx ? (int64_t)idx->names.size() : 0; }

const char *lfq_vcf_index_name(const lfq_vcf_index *idx, int64_t i)
{
    return idx && i >= 0 && (size_t)i < idx->names.size() ? idx->names[(size_t)i].c_str() : nullptr;
}

int lfq_vcf_index_query(const lfq_vcf_index *idx, const char *chrom, int64_t beg, int64_t end, const uint64_t **chunk_beg,
                        const uint64_t **chunk_end, int64_t *n_chunks)
{
    if (!idx || !chrom || !chunk_beg || !chunk_end || !n_chunks) {
        return LFQ_ERR_INVALID;
    }
    lfq_vcf_index *m = const_cast<lfq_vcf_index *>(idx);        /* (the result's storage) */
    lfq_tbx_query(m, chrom, beg, end);
    *chunk_beg = m->body.q_beg.data();
    *chunk_end = m->body.q_end.data();
    *n_chunks = (int64_t)m->body.q_beg.size();
    return LFQ_OK;
}

void lfq_vcf_index_free(lfq_vcf_index *idx) { delete idx; }

/* ---- a region through an index ----------------------------------------------------------------------------------------------------- */
int lfq_vcf_open_indexed(lfq_ctx *c, const uint8_t *comp, int64_t n_comp, const lfq_vcf_index *idx, const char *chrom, int64_t beg,
                         int64_t end, lfq_vcf **out, int *why_out, int64_t *bad_line_out)
{
    if (out) *out = nullptr;
    if (why_out) *why_out = LFQ_VC_OK;
    if (bad_line_out) *bad_line_out = 0;
    if (!c || !out || !idx || !chrom || n_comp < 0 || (n_comp > 0 && !comp)) {
        return LFQ_ERR_INVALID;
    }
    lfq_vcf_index *m = const_cast<lfq_vcf_index *>(idx);
    lfq_tbx_query(m, chrom, beg, end);
    if (m->body.q_beg.empty()) {
        return lfq_vcf_open(c, nullptr, 0, LFQ_VC_TABIX, out, why_out, bad_line_out);
    }
    /* the blocks from the one the first chunk begins in to the one the last chunk ends in, as they lie in the file */
    const uint64_t first = m->body.q_beg.front(), last = m->body.q_end.back();
    const int64_t c0 = (int64_t)(first >> 16), c1 = (int64_t)(last >> 16), o0 = (int64_t)(first & 0xffff), o1 = (int64_t)(last & 0xffff);
    if (c0 > c1 || c1 > n_comp) {
        return LFQ_ERR_INVALID;         /* (not this file's index) */
    }
    int64_t stop = c0, n_in_front = 0;  /* the blocks of [c0, c1) and, where the last chunk ends inside it, the one at c1 */
    while (stop < c1 || (stop == c1 && o1 > 0)) {
        const int64_t size = tbx_block_size(comp, n_comp, stop);
        if (size <= 0 || (stop < c1 && stop + size > c1)) {
            return LFQ_ERR_INVALID;
        }
        n_in_front += stop < c1 ? 1 : 0;
        stop += size;
    }
    const lfq_bgzf_result *res = nullptr;
    LFQ_TRY(lfq_bgzf_inflate(c, comp + c0, stop - c0, &res));
    const int64_t to = o1 > 0 ? res->data_off[n_in_front] + o1 : res->n_bytes;
    if (o0 > to || to > res->n_bytes) {
        return LFQ_ERR_INVALID;
    }
    return lfq_vcf_open(c, res->data + o0, to - o0, LFQ_VC_TABIX, out, why_out, bad_line_out);
}

}   /* extern "C" */
